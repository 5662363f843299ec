from .vec_greedy import VecGreedyPolicy  # noqa: F401
from .vec_cmaes import VecCmaesPolicy  # noqa: F401
from .vec_mcts_zero import VecMctsZeroPolicy  # noqa: F401
from .vec_mcts import VecMctsPolicy  # noqa: F401
from .device_ctree import DeviceClassicMCTS  # noqa: F401
