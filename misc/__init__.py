"""Drop-in import name ``misc.metric_util`` (``from misc.metric_util import MeanIoU`` at eval.py, train.py and
visualize.py).  The reference's own ``misc`` directory has no ``__init__.py`` and holds modules this repository does not
replace (``checkpoint_util``, ``tb_wrapper``): a regular package would hide them, so this one extends its search path
by every other ``misc`` directory on ``sys.path`` -- ``misc.metric_util`` resolves here, the rest where it lies."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
