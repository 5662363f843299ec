from .vec_greedy import VecGreedyPolicy  # noqa: F401
from .vec_cmaes import VecCmaesPolicy  # noqa: F401
from .vec_mcts_zero import VecMctsZeroPolicy  # noqa: F401
from .vec_mcts import VecMctsPolicy  # noqa: F401
from .device_ctree import DeviceClassicMCTS  # noqa: F401
from .vec_baselines import (VecLawnmowerPolicy, VecSpiralPolicy, VecRandomDiscretePolicy, VecRandomContinuousPolicy,  # noqa: F401
                            lawnmower_table, spiral_table, random_discrete_next, random_continuous_next, curve_resample_host,
                            curve_reduce_host)
from .mission_log import MissionLog, compare  # noqa: F401
