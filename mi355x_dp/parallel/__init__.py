from mi355x_dp.utils import hwqueues as _hwqueues

_hwqueues.ensure()  # before the first HIP call: compute / weight-gradient / comm streams on their own queues

from .ddp import DataParallel, plan_buckets  # noqa: E402,F401
from .optim import FlatAdamW, FlatLAMB, FlatLARS, FlatSGD  # noqa: E402,F401
from .ema import FlatEMA  # noqa: E402,F401
from .flat import FlatBuffers, FlatParams  # noqa: E402,F401
