from .selfplay import PrioritizedReplay, ReplayBuffer, SelfPlay  # noqa: F401
from .networks import DevicePolicyValueNet, PolicyValueNetwork  # noqa: F401
from .training import Trainer, one_cycle, pv_losses_host, sgd_clip_step_host  # noqa: F401
from .arena import Arena  # noqa: F401
