"""The reference's ``ScaleSpaceDetector`` (``cirtorch/features/scale_space_detector.py:47-175``) on the
engine's fused detector (rr_detect_scale_space): pyramid, response per level, strict 3-D extrema with
quadratic refinement, frames and the best N per image in one call, nothing read back.

The constructor keeps the reference's arguments.  Built: ``ScalePyramid`` without ``double_image``,
the responses ``BlobHessian``, ``CornerHarris``, ``CornerGFTT`` and ``BlobDoG``, ``ConvQuadInterp3d``
as ``nms_module`` (the default here; the reference's default ``ConvSoftArgmax3d`` keeps every voxel),
``PassLAF`` or ``LAFAffineShapeEstimator`` (Hessian-Affine; one pass, no iterated adaptation) as
``aff_module``, ``PassLAF`` or ``LAFOrienter`` as ``ori_module``, no mask.  Only strict
extrema become keypoints (the reference fills the list up with arbitrary voxels), each offset is
applied to its own axis, the scores carry no ``strict_maxima_bonus``, and an octave is not cut to
``num_features`` before the inside test: see include/rr.h.
"""

import torch.nn as nn

from .. import _ops
from ..geometry.subpix.spatial_soft_argmax import ConvQuadInterp3d
from ..geometry.transform.pyramid import ScalePyramid
from .affine_shape import LAFAffineShapeEstimator
from .orientation import LAFOrienter, PassLAF
from .responses import BlobDoG, BlobHessian, CornerGFTT, CornerHarris


class ScaleSpaceDetector(nn.Module):
    """
        Module for local feature detection, as close as possible to classical
        local feature detectors like Harris, Hessian-Affine or SIFT (DoG).
    """

    def __init__(self, num_features=500, mr_size=6.0, scale_pyr_module=None, resp_module=None, nms_module=None,
                 ori_module=None, aff_module=None, minima_are_also_good=False, scale_space_response=False):
        super(ScaleSpaceDetector, self).__init__()
        self.mr_size = mr_size
        self.num_features = num_features
        self.scale_pyr = ScalePyramid(3, 1.6, 15) if scale_pyr_module is None else scale_pyr_module
        self.resp = BlobHessian() if resp_module is None else resp_module
        self.nms = ConvQuadInterp3d(10.0) if nms_module is None else nms_module
        self.ori = PassLAF() if ori_module is None else ori_module
        self.aff = PassLAF() if aff_module is None else aff_module
        self.minima_are_also_good = minima_are_also_good
        self.scale_space_response = scale_space_response
        if type(self.scale_pyr) is not ScalePyramid:
            raise NotImplementedError("scale_pyr_module must be a ScalePyramid, got %s" % type(self.scale_pyr).__name__)
        if type(self.nms) is not ConvQuadInterp3d:
            raise NotImplementedError("nms_module must be a ConvQuadInterp3d, got %s" % type(self.nms).__name__)
        if type(self.aff) not in (PassLAF, LAFAffineShapeEstimator):
            raise NotImplementedError("aff_module must be PassLAF or LAFAffineShapeEstimator, got %s" % type(self.aff).__name__)
        if type(self.ori) not in (PassLAF, LAFOrienter):
            raise NotImplementedError("ori_module must be PassLAF or LAFOrienter, got %s" % type(self.ori).__name__)
        kinds = {BlobHessian: "hessian", CornerHarris: "harris", CornerGFTT: "gftt", BlobDoG: "dog"}
        if type(self.resp) not in kinds:
            raise NotImplementedError("resp_module must be BlobHessian, CornerHarris, CornerGFTT or BlobDoG, got %s"
                                      % type(self.resp).__name__)
        self._kind = kinds[type(self.resp)]
        if (self._kind == "dog") != bool(scale_space_response):
            raise ValueError("scale_space_response must be True for BlobDoG and False for the other responses")

    def detect(self, img, num_feats, mask=None):
        if mask is not None:
            raise NotImplementedError("masks are not built")
        sp = self.scale_pyr
        lafs, responses, _ = _ops.detect_scale_space(img, int(num_feats), self._kind, sp.levels, sp.sigma, sp.min_size,
                                                     self.mr_size, self.minima_are_also_good,
                                                     getattr(self.resp, "_k", 0.04))
        return responses, lafs

    def forward(self, img, mask=None):
        """
            Three stage local feature detection. First the location and scale of interest points are determined by
            detect function. Then affine shape and orientation.
        """
        responses, lafs = self.detect(img, self.num_features, mask)
        lafs = self.aff(lafs, img)
        lafs = self.ori(lafs, img)
        return lafs, responses
