from .matching import match_mnn, match_nn, match_smnn, match_snn  # noqa: F401
from .nms import NonMaximaSuppression2d, nms2d, nms3d  # noqa: F401
from .responses import (BlobDoG, BlobHessian, CornerGFTT, CornerHarris, dog_response, gftt_response,  # noqa: F401
                        harris_response, hessian_response)
from .affine_shape import LAFAffineShapeEstimator, PatchAffineShapeEstimator  # noqa: F401
from .laf import (denormalize_laf, ellipse_to_laf, extract_patches_from_pyramid, extract_patches_simple, get_laf_center,  # noqa: F401
                  get_laf_orientation, get_laf_scale, laf_from_center_scale_ori, laf_is_inside_image, make_upright,
                  normalize_laf, raise_error_if_laf_is_not_valid, scale_laf)
from .orientation import LAFOrienter, PassLAF, PatchDominantGradientOrientation  # noqa: F401
from .siftdesc import SIFTDescriptor, get_sift_bin_ksize_stride_pad, get_sift_pooling_kernel, sift_describe  # noqa: F401
from .scale_space_detector import ScaleSpaceDetector  # noqa: F401
from .hardnet import HardNet  # noqa: F401
from .sosnet import SOSNet  # noqa: F401
