"""`mesh-exporter` (threestudio/models/exporters/mesh_exporter.py:17-175, exporters/base.py:11-60): geometry.isosurface() -> an OBJ.

The reference's UV route (xatlas unwrapping, nvdiffrast rasterisation of the texture atlas, cv2 inpainting) is not part of this port, and
with `uv_method: "xatlas"` (the default, the reference's route) `save_uv: true` and `fmt: "obj-mtl"` are refused.  `uv_method: "face-cells"`
opts into an atlas of this port's own (csrc/atlas.hip): every face gets a triangle of its own in a grid of square cells, the texels of a cell
half are baked from the field at the nearest point of that face, a gutter of `uv_gutter` texels included, so bilinear lookups inside a face
never read another face's texel and no inpainting pass is needed.  It is NOT xatlas's atlas: 3 F texture vertices, no charts, and the
texture resolution per face is uniform rather than proportional to the face's area.  With it
  fmt "obj-mtl"          OBJ with `vt`, MTL, texture_kd (and texture_metallic / texture_roughness / texture_nrm if the material exports them)
  fmt "obj", save_uv     OBJ with `vt` and vertex colours
as export_obj_with_mtl / export_obj of the reference; the params of the ExporterOutput carry the reference's keys, the maps as uint8 HWC.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List

import torch

from .base import BaseObject
from .mesh import Mesh
from .registry import info, register, warn


@dataclass
class ExporterOutput:
    save_name: str
    save_type: str
    params: Dict[str, Any]


class Exporter(BaseObject):
    @dataclass
    class Config(BaseObject.Config):
        save_video: bool = False

    cfg: Config

    def configure(self, geometry, material, background) -> None:
        self.geometry, self.material, self.background = geometry, material, background

    def __call__(self, *args, **kwargs) -> List[ExporterOutput]:
        raise NotImplementedError


@register("dummy-exporter")
class DummyExporter(Exporter):
    def __call__(self, *args, **kwargs) -> List[ExporterOutput]:
        return []


NO_UV = ("needs a UV atlas: xatlas for the unwrapping and nvdiffrast for rasterising the texture, neither of which this port has. "
         'Supported: fmt: "obj" with save_uv: false (vertex colours), or uv_method: "face-cells" (a per-face atlas baked on the GPU)')
UV_METHODS = ("xatlas", "face-cells")
# material.export key -> the MTL map it becomes (mesh_exporter.py:120-131)
TEXTURE_MAPS = (("albedo", "map_Kd"), ("metallic", "map_Pm"), ("roughness", "map_Pr"), ("bump", "map_Bump"))


@register("mesh-exporter")
class MeshExporter(Exporter):
    @dataclass
    class Config(Exporter.Config):
        fmt: str = "obj-mtl"  # in ['obj-mtl', 'obj']
        save_name: str = "model"
        save_normal: bool = False
        save_uv: bool = True
        save_texture: bool = True
        texture_size: int = 1024
        texture_format: str = "jpg"
        xatlas_chart_options: dict = field(default_factory=dict)
        xatlas_pack_options: dict = field(default_factory=dict)
        context_type: str = "gl"
        uv_method: str = "xatlas"       # in ['xatlas' (the reference's, refused here), 'face-cells']
        # texels around every face's triangle that still carry that face.  1 is what bilinear sampling without mip-maps needs: a lookup at
        # (x, y) inside the lower triangle of a cell (side c, leg L = c - 3 g - 1) reads texel centres strictly within (x +- 1, y +- 1), whose
        # coordinate sums are < x + y + 2 <= c - g + 1, i.e. < c for g >= 1 as the sums are integers, and whose coordinates are > g - 1 >= 0:
        # the lower face's own texels (i + j + 1 < c), inside the cell.  The upper triangle is its mirror image (csrc/atlas.hip).
        uv_gutter: int = 1
        texture_chunk: int = 1 << 20    # points per field evaluation while baking

    cfg: Config

    def configure(self, geometry, material, background) -> None:
        super().configure(geometry, material, background)
        self.check_supported()

    def check_supported(self) -> None:
        if self.cfg.uv_method not in UV_METHODS:
            raise ValueError(f"Unsupported uv_method: {self.cfg.uv_method!r} (one of {', '.join(UV_METHODS)})")
        if self.cfg.fmt not in ("obj-mtl", "obj"):
            raise ValueError(f"Unsupported mesh export format: {self.cfg.fmt}")
        if self.cfg.uv_method == "xatlas":
            if self.cfg.fmt == "obj-mtl":
                raise NotImplementedError(f'mesh-exporter fmt "obj-mtl" {NO_UV}')
            if self.cfg.save_uv:
                raise NotImplementedError(f"mesh-exporter save_uv: true {NO_UV}")
        elif self.cfg.fmt == "obj-mtl" and self.cfg.save_texture and not self.cfg.save_uv:
            raise ValueError("save_uv must be True when save_texture is True")      # the reference's assert (mesh_exporter.py:74)

    def __call__(self) -> List[ExporterOutput]:
        self.check_supported()
        mesh = self.geometry.isosurface()
        return self.export_obj_with_mtl(mesh) if self.cfg.fmt == "obj-mtl" else self.export_obj(mesh)

    def unwrap_uv(self, mesh: Mesh) -> None:
        mesh.unwrap_uv(self.cfg.uv_method, self.cfg.uv_gutter, self.cfg.texture_size)

    def bake_textures(self, mesh: Mesh) -> Dict[str, Any]:
        """material.export over the atlas -> {key: uint8 [T,T,C] image}.  ops.atlas_bake gives every owned texel its 3-D point (the gutter
        included: that replaces the reference's cv2.inpaint); the field is evaluated at the owned texels only, in chunks, and every map
        the material returns is packed by the same kernel."""
        from . import ops

        T = self.cfg.texture_size
        gb_pos, face_id, _ = ops.atlas_bake(mesh.atlas, mesh.v_pos, mesh.t_pos_idx)
        owned = torch.nonzero(face_id.view(-1) >= 0).squeeze(1)
        points = gb_pos.view(-1, 3)[owned]
        images: Dict[str, Any] = {}
        chunk = max(1, int(self.cfg.texture_chunk))
        with torch.no_grad():
            for at in range(0, points.shape[0], chunk):     # no owned texel (an empty mesh): no map, the MTL's constant Kd
                p = points[at:at + chunk]
                geo_out = self.geometry.export(points=p)
                mat_out = self.material.export(points=p, **geo_out)
                for key, _ in TEXTURE_MAPS:
                    if key in mat_out:
                        values = mat_out[key].reshape(p.shape[0], -1).float()
                        if key not in images:
                            images[key] = torch.zeros((T, T, values.shape[1]), device=gb_pos.device, dtype=torch.uint8)
                        ops.atlas_pack_u8(values, owned[at:at + chunk], images[key])
        return images

    def export_obj_with_mtl(self, mesh: Mesh) -> List[ExporterOutput]:
        params = {"mesh": mesh, "save_mat": True, "save_normal": self.cfg.save_normal, "save_uv": self.cfg.save_uv, "save_vertex_color": False,
                  "map_Kd": None, "map_Ks": None, "map_Bump": None, "map_Pm": None, "map_Pr": None, "map_format": self.cfg.texture_format}
        if self.cfg.save_uv:
            self.unwrap_uv(mesh)
        if self.cfg.save_texture:
            info("Exporting textures ...")
            if not self.cfg.save_uv:
                raise ValueError("save_uv must be True when save_texture is True")
            images = self.bake_textures(mesh)
            if "albedo" not in images:
                warn("save_texture is True but no albedo texture found, using default white texture")
            for key, name in TEXTURE_MAPS:
                if key in images:
                    params[name] = images[key]
        return [ExporterOutput(save_name=f"{self.cfg.save_name}.obj", save_type="obj", params=params)]

    def export_obj(self, mesh: Mesh) -> List[ExporterOutput]:
        params = {"mesh": mesh, "save_mat": False, "save_normal": self.cfg.save_normal, "save_uv": self.cfg.save_uv, "save_vertex_color": False,
                  "map_Kd": None, "map_Ks": None, "map_Bump": None, "map_Pm": None, "map_Pr": None, "map_format": self.cfg.texture_format}
        if self.cfg.save_uv:
            self.unwrap_uv(mesh)
        if self.cfg.save_texture:
            info("Exporting textures ...")
            geo_out = self.geometry.export(points=mesh.v_pos)
            mat_out = self.material.export(points=mesh.v_pos, **geo_out)
            if "albedo" in mat_out:
                mesh.set_vertex_color(mat_out["albedo"])
                params["save_vertex_color"] = True
            else:
                warn("save_texture is True but no albedo texture found, not saving vertex color")
        return [ExporterOutput(save_name=f"{self.cfg.save_name}.obj", save_type="obj", params=params)]
