"""`mesh-exporter` (threestudio/models/exporters/mesh_exporter.py:17-175, exporters/base.py:11-60): geometry.isosurface() -> an OBJ with
vertex colours.  The UV route (xatlas unwrapping, nvdiffrast rasterisation of the texture atlas, cv2 inpainting) is not part of this
port: `save_uv: true` and `fmt: "obj-mtl"` are refused, nothing else is written in their place.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List

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
         'Supported: fmt: "obj" with save_uv: false (vertex colours)')


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

    cfg: Config

    def configure(self, geometry, material, background) -> None:
        super().configure(geometry, material, background)
        self.check_supported()

    def check_supported(self) -> None:
        if self.cfg.fmt == "obj-mtl":
            raise NotImplementedError(f'mesh-exporter fmt "obj-mtl" {NO_UV}')
        if self.cfg.fmt != "obj":
            raise ValueError(f"Unsupported mesh export format: {self.cfg.fmt}")
        if self.cfg.save_uv:
            raise NotImplementedError(f"mesh-exporter save_uv: true {NO_UV}")

    def __call__(self) -> List[ExporterOutput]:
        self.check_supported()
        return self.export_obj(self.geometry.isosurface())

    def export_obj(self, mesh: Mesh) -> List[ExporterOutput]:
        params = {"mesh": mesh, "save_mat": False, "save_normal": self.cfg.save_normal, "save_uv": self.cfg.save_uv, "save_vertex_color": False,
                  "map_Kd": None, "map_Ks": None, "map_Bump": None, "map_Pm": None, "map_Pr": None, "map_format": self.cfg.texture_format}
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
