"""ssme_amd: MI355X-native bootstrap-particle-filter core behind ssme's BSFilter<>::filter().

Python host mirror of the reference's filter interface over the C ABI (include/ssme_pf.h).
"""
from .filters import *  # noqa: F401,F403
from . import _capi  # noqa: F401
from ._capi import ROUTE_TILED, ROUTE_SERIES_LANE, ROUTE_SERIES_PAIR, ROUTE_LW_SERIES  # noqa: F401  (series_route() of the banks and the Liu-West filters)

__version__ = "0.1.0"
