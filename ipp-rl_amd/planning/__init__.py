from .vec_greedy import VecGreedyPolicy  # noqa: F401
