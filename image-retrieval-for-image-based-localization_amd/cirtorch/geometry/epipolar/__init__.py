from .essential import (decompose_essential_matrix, essential_from_fundamental, essential_from_Rt,  # noqa: F401
                        motion_from_essential, motion_from_essential_choose_solution, relative_camera_motion,
                        run_5point)
from .fundamental import (compute_correspond_epilines, find_fundamental, fundamental_from_essential,  # noqa: F401
                          normalize_points, normalize_transformation)
from .metrics import sampson_epipolar_distance, symmetrical_epipolar_distance  # noqa: F401
from .projection import (KRt_from_projection, depth, intrinsics_like, projection_from_KRt,  # noqa: F401
                         projections_from_fundamental, scale_intrinsics)
from .triangulation import triangulate_points  # noqa: F401
