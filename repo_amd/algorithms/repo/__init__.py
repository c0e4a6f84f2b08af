from .dreamer import Dreamer
from .dreamer_mt import MultitaskDreamer
from .models.decoder import ContinuationModel
from .models.utils import InverseDynamicsModel
from .repo import RePo
from .repo_adapt import CalibratedRePo, FinetunedRePo
from .repo_mt import MultitaskRePo
from .tia import TIA

__all__ = ["Dreamer", "RePo", "TIA", "FinetunedRePo", "CalibratedRePo", "MultitaskDreamer", "MultitaskRePo",
           "InverseDynamicsModel", "ContinuationModel"]
