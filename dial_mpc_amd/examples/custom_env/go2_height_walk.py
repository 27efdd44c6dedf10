"""Custom-environment example: the Go2 walking forward at ``vx`` while it holds its trunk at ``height``, with a reward written
in HIP (go2_height_walk.hip) and compiled into a task plugin on first use.

    python -m dial_mpc_amd.core.dial_core --custom-env dial_mpc_amd.examples.custom_env.go2_height_walk \\
        --config dial_mpc_amd/examples/custom_env/go2_height_walk.yaml
"""
from dataclasses import dataclass

import numpy as np

from dial_mpc_amd.envs import register_config, register_environment
from dial_mpc_amd.envs.custom_env import CustomEnv
from dial_mpc_amd.envs.unitree_go2_env import UnitreeGo2EnvConfig


@dataclass
class Go2HeightWalkConfig(UnitreeGo2EnvConfig):
    vx: float = 0.6
    height: float = 0.3
    w_vel: float = 1.0
    w_height: float = 10.0
    w_upright: float = 1.0
    w_ctrl: float = 1e-5


class Go2HeightWalkEnv(CustomEnv):
    model_path = "../../models/unitree_go2/mjx_scene_force.json"
    reward_hip = "go2_height_walk.hip"
    user_params = ("vx", "height", "w_vel", "w_height", "w_upright", "w_ctrl")

    def __init__(self, config: Go2HeightWalkConfig):
        super().__init__(config)
        self.joint_range = np.array(  # the walking envs' sampling range (unitree_go2_env.py)
            [[-0.5, 0.5], [0.4, 1.4], [-2.3, -0.85],
             [-0.5, 0.5], [0.4, 1.4], [-2.3, -0.85],
             [-0.5, 0.5], [0.4, 1.4], [-2.3, -1.3],
             [-0.5, 0.5], [0.4, 1.4], [-2.3, -1.3]])


register_config("go2_height_walk", Go2HeightWalkConfig)
register_environment("go2_height_walk", Go2HeightWalkEnv)
