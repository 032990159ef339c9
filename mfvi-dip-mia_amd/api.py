"""Public surface."""
from . import _lib
from ._build import build
from .program import Plan, Program, skip_program
from . import engine, sharding
from .fitbatch import FitBatch
from . import runner
from .nets import Concat, get_net, skip

__all__ = ["build", "FitBatch", "Plan", "Program", "skip_program", "_lib", "engine", "sharding", "runner", "Concat", "get_net", "skip", "MeanFieldVI", "FusedNet", "Conv2dRT", "Conv2dLRT",
           "gaussian_nll", "gaussian_nll_inpainting", "uncert_regression_gal", "uceloss", "Downsampler", "lanczos_taps", "FastRadonTransform", "CtVolume", "InpaintBatch", "SiblingBatch", "BatchBook", "tv_loss", "prune_weights_ffg", "prune_remove"]


def __getattr__(name):          # bayes.py needs torch.nn at import: keep `import mfvi_dip_mia_amd` light
    if name in ("MeanFieldVI", "FusedNet", "Conv2dRT", "Conv2dLRT", "gaussian_nll", "gaussian_nll_inpainting", "uncert_regression_gal", "prune_weights_ffg", "prune_remove"):
        from . import bayes
        return getattr(bayes, name)
    if name == "uceloss":
        from .calibration import uceloss
        return uceloss
    if name in ("Downsampler", "lanczos_taps"):
        from . import downsampler
        return getattr(downsampler, name)
    if name == "FastRadonTransform":
        from . import radon
        return radon.FastRadonTransform
    if name == "CtVolume":
        from .ctvolume import CtVolume
        return CtVolume
    if name == "InpaintBatch":
        from .inpaintbatch import InpaintBatch
        return InpaintBatch
    if name == "SiblingBatch":
        from .siblingbatch import SiblingBatch
        return SiblingBatch
    if name == "BatchBook":
        from .batchbook import BatchBook
        return BatchBook
    if name == "tv_loss":
        from .tv import tv_loss
        return tv_loss
    raise AttributeError(name)
