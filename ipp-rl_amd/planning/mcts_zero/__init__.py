from .selfplay import PrioritizedReplay, ReplayBuffer, SelfPlay  # noqa: F401
