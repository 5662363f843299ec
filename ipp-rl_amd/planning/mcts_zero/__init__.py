from .selfplay import ReplayBuffer, SelfPlay  # noqa: F401
