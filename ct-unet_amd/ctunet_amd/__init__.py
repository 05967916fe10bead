"""ctunet_amd -- MI355X-native 3D U-Net path behind the ctunet model-class API.

The kernels live in libctunet_hip.so (C ABI: include/ctunet_hip.h); this package is the host
side that mirrors ``ctunet.pytorch.models`` / ``ctunet.utilities`` / ``ctunet.pytorch.ProblemHandler``
for the hot path only.  Importing it does not need a GPU; running a model does.
"""
from . import _lib  # noqa: F401
from . import lr_scheduler  # noqa: F401
from . import mesh  # noqa: F401
from . import metrics  # noqa: F401
from . import optim  # noqa: F401
from . import postprocess  # noqa: F401
from . import preprocess  # noqa: F401
from . import resample  # noqa: F401
from . import sampling  # noqa: F401
from . import registration  # noqa: F401
from . import simplify  # noqa: F401
from .inference import Prediction, predict_volume  # noqa: F401
from .datasets import FlapRec2OTrainDataset, FlapRecPatchDataset, FlapRecWShapePrior2OTrainDataset  # noqa: F401
from .loss_scale import DynamicLossScale  # noqa: F401
from .losses import LossSpec, boundary_map, seg_loss  # noqa: F401
from .models import (UNet, UNet4_2IC, UNet4b1i3o, UNet4b2i3o, UNet5b2i3o, UNetDO, UNetSP, UNetSPSmall,  # noqa: F401
                     recAE_v2_fixed)
from .transforms import (FlapRecTransform, RandomDilate, RandomSpatial, SaltAndPepper, SkullRandomDefect,  # noqa: F401
                         SkullRandomHole, cranioplasty_transform, flap_rec_transform, realistic_cranioplasty_transform)

__all__ = ["UNet", "UNet4b2i3o", "UNet5b2i3o", "UNet4b1i3o", "UNetSP", "UNetSPSmall", "UNetDO", "recAE_v2_fixed",
           "UNet4_2IC", "DynamicLossScale", "predict_volume", "Prediction",
           "SkullRandomHole", "SaltAndPepper", "FlapRecTransform", "flap_rec_transform", "RandomSpatial",
           "cranioplasty_transform", "SkullRandomDefect", "RandomDilate", "realistic_cranioplasty_transform", "FlapRecWShapePrior2OTrainDataset", "FlapRec2OTrainDataset", "metrics", "postprocess", "preprocess", "resample", "registration", "mesh", "lr_scheduler",
           "optim", "simplify", "LossSpec", "seg_loss", "boundary_map", "sampling", "FlapRecPatchDataset"]
