"""Reference path ``cirtorch/modules/pools.py`` (POOLING_LAYERS at :200-207).

GeM / MAC / SPoC / GeMmp and the regional ROIpool (``Rpool``) run on the
engine.  RMAC keeps raising: upstream its region loop is mis-indented
(``pools.py:105-113``), so it pools a single region; ``Rpool(MAC())`` is the
correct R-MAC.
"""

from ..layers.pooling import GeM, GeMmp, MAC, Rpool, SPoC  # noqa: F401


def RMAC(*args, **kwargs):
    raise NotImplementedError("RMAC is not built: the upstream region loop is mis-indented (it pools one region "
                              "only); use Rpool(MAC()) / POOLING_LAYERS['ROIpool'](rpool=MAC()), the correct R-MAC")


POOLING_LAYERS = {
    "MAC": MAC,
    "SPoC": SPoC,
    "GeM": GeM,
    "GeMmp": GeMmp,
    "RMAC": RMAC,
    "ROIpool": Rpool,
}
