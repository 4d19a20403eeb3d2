"""Params / Camera mirrors (reference: src/params.jl:58-82, src/camera.jl:1-67).
Only the fields the hot path reads."""
from dataclasses import dataclass


@dataclass
class Params:
    stereo: bool = False
    max_nb_keypoints: int = 1000
    max_distance: int = 35
    max_ktl_distance: float = 1.0
    pyramid_levels: int = 3
    pyramid_sigma: float = 1.0
    window_size: int = 9
    max_reprojection_error: float = 3.0
    min_cov_score: int = 25
    do_local_matching: bool = False
    filtering_ratio: float = 0.9             # params.jl:71: map_filtering! removes a key-frame when more than this share of its 3-D points has > 4 observers
    map_filtering: bool = False              # params.jl:72
    do_local_bundle_adjustment: bool = True
    max_projection_distance: float = 2.0     # params.jl:75: gate of the local-map match, px
    max_descriptor_distance: float = 0.35    # params.jl:76: share of the 256 descriptor bits
    initial_parallax: float = 20.0           # params.jl:66: px; check_ready_for_init! and the parallax rule of check_new_kf_required


@dataclass
class Camera:
    fx: float
    fy: float
    cx: float
    cy: float
    height: int
    width: int

    def project(self, point):
        """camera.jl:62-67: (x, y, z) -> (y, x) pixel."""
        inv_z = 1.0 / point[2]
        return (self.fy * point[1] * inv_z + self.cy, self.fx * point[0] * inv_z + self.cx)

    @property
    def intrinsics(self):
        return (self.fx, self.fy, self.cx, self.cy)
