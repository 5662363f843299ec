from .selfplay import PrioritizedReplay, ReplayBuffer, SelfPlay  # noqa: F401
from .networks import DevicePolicyValueNet, PolicyValueNetwork  # noqa: F401
