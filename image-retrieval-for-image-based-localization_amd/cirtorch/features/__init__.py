from .matching import match_mnn, match_nn, match_smnn, match_snn  # noqa: F401
from .nms import NonMaximaSuppression2d, nms2d, nms3d  # noqa: F401
from .responses import (BlobHessian, CornerGFTT, CornerHarris, gftt_response, harris_response,  # noqa: F401
                        hessian_response)
