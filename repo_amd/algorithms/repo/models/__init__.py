from .actor_critic import ActorModel, ValueModel
from .decoder import ContinuationModel, ObservationModel, RewardModel, TIAObservationModel, VisualObservationModel
from .encoder import Encoder, VisualEncoder
from .rssm import TransitionModel
from .utils import FlatAdam, InverseDynamicsModel, bottle

__all__ = ["ActorModel", "ValueModel", "ObservationModel", "RewardModel", "ContinuationModel", "VisualObservationModel", "TIAObservationModel", "Encoder",
           "VisualEncoder", "TransitionModel", "InverseDynamicsModel", "FlatAdam", "bottle"]
