"""One ASD_GEMM_TRACE line per GEMM / convolution launch of the four network passes of csrc/net.hip, on the small configurations of
tests/test_gpu_net_abi.py (eager, tune = 0, the committed plan table):

    [ASD_HIP_LIB=/path/to/libasd_hip.so] python tools/net_schedule_trace.py --out DIR        (GPU box)

writes DIR/{unet_fwd,vae_enc_fwd,vae_enc_bwd,vae_dec_fwd}.trace and prints line count and sha256 of each.  One library per process
(ASD_HIP_LIB): run it once per build and compare the files — a refactor of the schedules leaves them byte-identical
(profiles/net_schedule_identity.txt).  The trace names shape, tile, split and record mode of a launch (gn=0 none, 1 forward records,
2 backward form), not addresses."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["ASD_GEMM_TRACE"] = "1"      # read by the library at its first launch

import torch  # noqa: E402

from scaledreamer_amd._lib import WeightInfo, check, i32, lib  # noqa: E402
from scaledreamer_amd.diffusion import hip_ops as H  # noqa: E402,F401  (pushes the committed plans into the library)
from scaledreamer_amd.diffusion import weights as W  # noqa: E402
from scaledreamer_amd.diffusion.engine import unet_desc  # noqa: E402
from scaledreamer_amd.diffusion.vae_hip import vae_desc  # noqa: E402


def make(kind, desc, packed):
    l, h = lib(), C.c_void_p()
    check(getattr(l, f"asd_{kind}_create")(C.byref(desc), C.byref(h)))
    n = getattr(l, f"asd_{kind}_num_weights")(h)
    info, keep, ptrs = WeightInfo(), [], (C.c_void_p * n)()
    for i in range(n):
        check(getattr(l, f"asd_{kind}_weight_info")(h, i32(i), C.byref(info)))
        keep.append(packed[info.name.decode()].to(device="cuda", dtype=torch.float16).contiguous())
        ptrs[i] = keep[-1].data_ptr()
    check(getattr(l, f"asd_{kind}_bind_weights")(h, ptrs, i32(n)))
    return h, keep


class Stderr:
    """the library traces to the C stderr: point file descriptor 2 at a file for the duration of one pass"""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        fd = os.open(self.path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.dup2(fd, 2)
        os.close(fd)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        os.dup2(self.saved, 2)
        os.close(self.saved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    l, p = lib(), lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = dict(device="cuda")
    path = lambda name: os.path.join(a.out, name + ".trace")  # noqa: E731

    ucfg = W.UNetConfig(model_channels=128, num_head_channels=64, context_dim=128)
    B, hw, n_ctx = 3, 32, 77
    h, keep = make("unet", unet_desc(ucfg), W.pack_unet(W.gen_params(W.unet_layout(ucfg)[0], seed=21), ucfg))
    x, ctx = torch.zeros(B, hw, hw, 32, dtype=torch.float16, **dev), torch.zeros(B, 80, 128, dtype=torch.float16, **dev)
    t, eps = torch.tensor([815.0, 20.0, 999.0], **dev), torch.empty(B, hw, hw, 4, **dev)
    nb = l.asd_unet_workspace_bytes(h, i32(B), i32(hw), i32(hw), i32(n_ctx), i32(1), i32(0))
    ws = torch.empty(nb, dtype=torch.uint8, **dev)
    with Stderr(path("unet_fwd")):
        check(l.asd_unet_fwd(h, p(x), p(t), p(ctx), None, i32(B), i32(hw), i32(hw), i32(n_ctx), i32(1), p(ws), C.c_int64(nb), p(eps), i32(0), st))
    l.asd_unet_destroy(h)

    import numpy as np

    g = np.load(os.path.join(ROOT, "tests", "golden", "diffusion_vae_small.npz"))       # its configuration and shape only
    ch, nrb, zc = (int(v) for v in g["cfg"])
    vcfg = W.VAEConfig(ch=ch, num_res_blocks=nrb, z_channels=zc, ch_mult=tuple(int(v) for v in g["ch_mult"]))
    B, res = int(g["batch"]), int(g["res"])
    h, keep = make("vae_enc", vae_desc(vcfg), W.pack_vae_encoder(W.gen_params(W.vae_encoder_layout(vcfg)[0], 6), vcfg))
    x, m = torch.zeros(B, res, res, 32, dtype=torch.float16, **dev), torch.empty(B, res // 8, res // 8, 8, **dev)
    gm, dx = torch.zeros(B, res // 8, res // 8, 8, **dev), torch.empty(B, res, res, 32, dtype=torch.float16, **dev)
    nb = l.asd_vae_enc_workspace_bytes(h, i32(B), i32(res), i32(res), i32(0))
    ws = torch.empty(nb, dtype=torch.uint8, **dev)
    with Stderr(path("vae_enc_fwd")):
        check(l.asd_vae_enc_fwd(h, p(x), i32(B), i32(res), i32(res), p(ws), C.c_int64(nb), p(m), i32(0), st))
    with Stderr(path("vae_enc_bwd")):
        check(l.asd_vae_enc_bwd(h, p(gm), i32(B), i32(res), i32(res), p(ws), C.c_int64(nb), p(dx), i32(0), st))
    l.asd_vae_enc_destroy(h)

    hl = 8
    h, keep = make("vae_dec", vae_desc(vcfg), W.pack_vae_decoder(W.gen_params(W.vae_decoder_layout(vcfg)[0], 6), vcfg))
    z, img = torch.zeros(B, hl, hl, 32, dtype=torch.float16, **dev), torch.empty(B, 8 * hl, 8 * hl, 32, dtype=torch.float16, **dev)
    nb = l.asd_vae_dec_workspace_bytes(h, i32(B), i32(hl), i32(hl), i32(0))
    ws = torch.empty(nb, dtype=torch.uint8, **dev)
    with Stderr(path("vae_dec_fwd")):
        check(l.asd_vae_dec_fwd(h, p(z), i32(B), i32(hl), i32(hl), p(ws), C.c_int64(nb), p(img), i32(0), st))
    l.asd_vae_dec_destroy(h)
    del keep

    for name in ("unet_fwd", "vae_enc_fwd", "vae_enc_bwd", "vae_dec_fwd"):
        data = open(path(name), "rb").read()
        lines = data.splitlines()
        assert lines and all(ln.startswith(b"ASD_GEMM ") for ln in lines), name
        print(f"{name}: {len(lines)} lines, sha256 {hashlib.sha256(data).hexdigest()}, "
              f"gn modes {sorted(set(ln.rsplit(b'gn=', 1)[1].decode() for ln in lines))}")


if __name__ == "__main__":
    main()
