from .selfplay import PrioritizedReplay, ReplayBuffer, ReplayWindow, SelfPlay  # noqa: F401
from .networks import DevicePolicyValueNet, PolicyValueNetwork  # noqa: F401
from .training import Trainer, one_cycle, pv_losses_host, sgd_clip_step_host  # noqa: F401
from .arena import Arena  # noqa: F401
from .learn import Learner, exploration_schedule, off_policy_window_size  # noqa: F401
