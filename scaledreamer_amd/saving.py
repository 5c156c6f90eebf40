"""`SaverMixin`: the image grids and frame sequences of the validation / test passes (threestudio/utils/saving.py:22-54 save dir,
:77-109 get_rgb_image_, :179-221 get_grayscale_image_, :255-328 get_image_grid_ / save_image_grid, :395-431 save_img_sequence).

A grid is composed from float panels to bytes in one launch (ops.image_grid: asd_image_minmax_f32 + asd_image_grid_u8) when its
panels are device tensors; host tensors go through `grid_cpu`, a torch restatement of the same fp32 arithmetic that the CPU suite pins
against the reference's bytes.  Only what those passes use is ported: equal-sized `rgb` and `grayscale` panels without a colour map.
cv2's jet table and fixed-point resize cannot be reproduced here, so other colour maps, `uv` panels and panels of unequal size are
refused.  PNGs are written with PIL in RGB order — the reference holds BGR in memory only because cv2.imwrite takes BGR.
"""
from __future__ import annotations

import os
import re
from typing import Any, List, Optional, Sequence, Tuple

import torch

from .registry import debug, warn

Panel = Tuple[str, torch.Tensor, float, float, bool]       # (kind, src [B,H,W(,3)], lo, hi, normalize): the argument of ops.image_grid

DEFAULT_RGB_KWARGS = {"data_format": "HWC", "data_range": (0, 1)}
DEFAULT_UV_KWARGS = {"data_format": "HWC", "data_range": (0, 1), "cmap": "checkerboard"}
DEFAULT_GRAYSCALE_KWARGS = {"data_range": None, "cmap": "jet"}
DEFAULT_GRID_KWARGS = {"align": "max"}

_warned_no_imageio = False


def grid_cpu(panels: Sequence[Panel]) -> torch.Tensor:
    """ops.image_grid restated with torch on any device (include/asd_hip.h asd_image_grid_u8): per value in fp32,
    grayscale: normalize by the image's own min / max if asked, then nan_to_num; both kinds: clip to [lo, hi],
    (v - lo) / (hi - lo) * 255, truncate.  A NaN of an rgb panel is written as 0."""
    cols = []
    for kind, src, lo, hi, normalize in panels:
        v = src.detach().to(torch.float32)
        lo_t, hi_t = (torch.tensor(float(x), dtype=torch.float32, device=v.device) for x in (lo, hi))
        if kind == "grayscale":
            if normalize:
                flat = v.reshape(v.shape[0], -1)
                mn, mx = (f(flat, dim=1).view(-1, 1, 1) for f in (torch.amin, torch.amax))
                v = (v - mn) / (mx - mn)
            v = torch.nan_to_num(v)                    # NaN -> 0, +-inf -> +-FLT_MAX
        else:
            v = torch.where(torch.isnan(v), lo_t, v)   # fmaxf(NaN, lo) = lo
        v = torch.minimum(torch.maximum(v, lo_t), hi_t)
        u = (v - lo_t) / (hi_t - lo_t) * 255.0
        b = u.to(torch.int32).to(torch.uint8)          # truncation; u is in [0, 255]
        cols.append(b[..., None].expand(*b.shape, 3) if kind == "grayscale" else b)
    return torch.cat(cols, dim=2).contiguous()


def panels_of(cols: Sequence[dict], batched: bool = False) -> List[Panel]:
    """the reference's `{"type", "img", "kwargs"}` dicts of one grid row -> panels [B,H,W(,3)] (B = 1 unless `batched`: then every img
    carries a leading batch dimension).  Refuses what is not ported, each with its own message."""
    out: List[Panel] = []
    for col in cols:
        kind = col["type"]
        assert kind in ["rgb", "uv", "grayscale"]
        if kind == "uv":
            raise NotImplementedError("image grid: 'uv' panels (checkerboard / colour UV maps) are not ported")
        kw = dict(DEFAULT_RGB_KWARGS if kind == "rgb" else DEFAULT_GRAYSCALE_KWARGS)
        kw.update(col.get("kwargs") or {})
        img = col["img"]
        if not torch.is_tensor(img):
            img = torch.as_tensor(img)
        if not img.is_floating_point():
            raise TypeError(f"image grid: panels are float images (got {img.dtype})")
        if not batched:
            img = img[None]
        if kind == "rgb":
            assert kw["data_format"] in ["CHW", "HWC"]
            if kw["data_format"] == "CHW":
                img = img.permute(0, 2, 3, 1)
            if img.dim() != 4 or img.shape[-1] != 3:
                raise ValueError(f"image grid: an rgb panel has 3 channels (got {tuple(img.shape[1:])})")
            lo, hi = kw["data_range"]
            out.append(("rgb", img, float(lo), float(hi), False))
        else:
            if kw["cmap"] is not None:
                raise NotImplementedError(f"image grid: colour map {kw['cmap']!r} is not ported (cv2's jet table, matplotlib's magma and "
                                          "spectral): pass cmap=None for a grey panel")
            if img.dim() != 3:
                raise ValueError(f"image grid: a grayscale panel is [H,W] (got {tuple(img.shape[1:])})")
            if kw["data_range"] is None:               # own min / max
                out.append(("grayscale", img, 0.0, 1.0, True))
            else:
                lo, hi = kw["data_range"]
                out.append(("grayscale", img, float(lo), float(hi), False))
    if not out:
        raise ValueError("image grid: no panels")
    first = tuple(out[0][1].shape[:3])
    for j, p in enumerate(out):
        if tuple(p[1].shape[:3]) != first:
            raise ValueError(f"image grid: panels of unequal size ({tuple(p[1].shape[1:3])} at column {j}, {first[1:]} at column 0) are not "
                             "resized: cv2.resize's fixed-point interpolation is not ported")
    return out


def compose(panels: Sequence[Panel]) -> torch.Tensor:
    """uint8 [B, H, P W, 3]: on the device when any panel lives there, else the CPU restatement"""
    devices = [p[1].device for p in panels if p[1].is_cuda]
    if not devices:
        return grid_cpu(panels)
    from . import ops

    return ops.image_grid([(k, src.to(devices[0]), lo, hi, nz) for k, src, lo, hi, nz in panels])


def write_png(path: str, img: torch.Tensor) -> str:
    """uint8 [H,W,3] RGB -> file (PIL, as mesh._save_map)"""
    import numpy as np
    from PIL import Image

    Image.fromarray(np.ascontiguousarray(img.detach().cpu().numpy())).save(path)
    return path


def _gif_blocks(data: bytes):
    """(logical screen descriptor, global colour table, graphic control extension or None, image descriptor, local colour table, image data)
    of a single-image GIF"""
    lsd = data[6:13]
    pos = 13
    gct = b""
    if lsd[4] & 0x80:
        n = 3 << ((lsd[4] & 7) + 1)
        gct, pos = data[pos:pos + n], pos + n
    gce = None

    def sub_blocks(at):                 # past a chain of size-prefixed sub-blocks and its terminator
        while data[at]:
            at += 1 + data[at]
        return at + 1

    while data[pos] != 0x2C:
        if data[pos] != 0x21:
            raise ValueError("write_gif: unexpected block in a frame's GIF encoding")
        end = sub_blocks(pos + 2)
        if data[pos + 1] == 0xF9:
            gce = data[pos:end]
        pos = end
    desc, pos = data[pos:pos + 10], pos + 10
    lct = b""
    if desc[9] & 0x80:
        n = 3 << ((desc[9] & 7) + 1)
        lct, pos = data[pos:pos + n], pos + n
    end = sub_blocks(pos + 1)           # LZW minimum code size, then the data sub-blocks
    return lsd, gct, gce, desc, lct, data[pos:end]


def write_gif(path: str, frames, fps: float) -> str:
    """PIL images -> an animated GIF with exactly one image block per frame, looping.  PIL encodes every frame (its own quantiser and LZW);
    the container is assembled here, because PIL's multi-frame writer folds a frame that equals its predecessor into the predecessor's
    duration — the first and last view of a test orbit (azimuth 0 and 360) are such a pair, and a sequence has one frame per view."""
    import io
    import struct

    delay = max(1, round(100.0 / fps))          # hundredths of a second
    out = bytearray()
    for k, frame in enumerate(frames):
        buf = io.BytesIO()
        frame.save(buf, format="GIF")
        lsd, gct, gce, desc, lct, image = _gif_blocks(buf.getvalue())
        if k == 0:
            out += b"GIF89a" + lsd[:4] + bytes([lsd[4] & 0x70, 0, 0])               # no global colour table: every frame brings its own
            out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00"                   # loop forever
        elif lsd[:4] != bytes(out[6:10]):
            raise ValueError("write_gif: frames of unequal size")
        table = lct or gct
        bits = (desc[9] & 7) if lct else (lsd[4] & 7)
        transparent = gce is not None and bool(gce[3] & 1)
        out += b"\x21\xF9\x04" + bytes([0x04 | (1 if transparent else 0)]) + struct.pack("<H", delay) + bytes([gce[6] if transparent else 0, 0])
        out += desc[:9] + bytes([(desc[9] & 0x40) | 0x80 | bits]) + table + image
    out += b"\x3B"
    with open(path, "wb") as fh:
        fh.write(bytes(out))
    return path


class SaverMixin:
    _save_dir: Optional[str] = None

    def set_save_dir(self, save_dir: str):
        self._save_dir = save_dir

    def get_save_dir(self):
        if self._save_dir is None:
            raise ValueError("Save dir is not set")
        return self._save_dir

    def get_save_path(self, filename):
        save_path = os.path.join(self.get_save_dir(), filename)
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
        return save_path

    def get_image_grid_(self, imgs, align=DEFAULT_GRID_KWARGS["align"]) -> torch.Tensor:
        """uint8 [rows H, P W, 3] in RGB order; a list of lists is stacked as rows"""
        if not (align in ("max", "min") or isinstance(align, int)
                or (isinstance(align, tuple) and len(align) == 2 and all(isinstance(a, int) for a in align))):
            raise ValueError(f"Unsupported image grid align: {align}, should be min, max, int or (int, int)")
        if isinstance(imgs[0], list):
            rows = [self.get_image_grid_(row, align) for row in imgs]
            if len({r.shape[1] for r in rows}) != 1:
                raise ValueError(f"image grid: rows of unequal width ({[r.shape[1] for r in rows]}) cannot be stacked")
            dev = next((r.device for r in rows if r.is_cuda), rows[0].device)
            return torch.cat([r.to(dev) for r in rows], dim=0)
        return compose(panels_of(imgs))[0]

    def save_image_grid(self, filename, imgs, align=DEFAULT_GRID_KWARGS["align"], name: Optional[str] = None, step: Optional[int] = None,
                        texts: Optional[List[Any]] = None) -> str:
        if texts is not None or name is not None:
            debug("save_image_grid: the text overlay and wandb logging are not ported; texts / name / step are ignored")
        return write_png(self.get_save_path(filename), self.get_image_grid_(imgs, align=align))

    def save_img_sequence(self, filename, img_dir, matcher, save_format="mp4", fps=30, name: Optional[str] = None, step: Optional[int] = None,
                          multithreaded: bool = False) -> str:
        """the frames of img_dir whose names match, ordered by the integer the matcher captures, as one gif (write_gif) or mp4 (imageio).
        Without imageio an mp4 request is answered with the GIF beside the requested name, and that path is returned."""
        global _warned_no_imageio
        import numpy as np
        from PIL import Image

        assert save_format in ["gif", "mp4"]
        if not filename.endswith(save_format):
            filename += f".{save_format}"
        save_path = self.get_save_path(filename)
        matcher = re.compile(matcher)
        img_dir = os.path.join(self.get_save_dir(), img_dir)
        names = sorted((f for f in os.listdir(img_dir) if matcher.search(f)), key=lambda f: int(matcher.search(f).groups()[0]))
        if not names:
            raise ValueError(f"save_img_sequence: no file of {img_dir} matches {matcher.pattern!r}")
        frames = []
        for f in names:
            with Image.open(os.path.join(img_dir, f)) as im:
                frames.append(im.convert("RGB").copy())
        if save_format == "mp4":
            try:
                import imageio
            except ImportError:
                imageio = None
            if imageio is not None:
                imageio.mimsave(save_path, [np.asarray(f) for f in frames], fps=fps)
                return save_path
            if not _warned_no_imageio:
                warn("save_img_sequence: imageio is not installed, writing a GIF instead of the mp4")
                _warned_no_imageio = True
            save_path = save_path[: -len("mp4")] + "gif"
        return write_gif(save_path, frames, fps)
