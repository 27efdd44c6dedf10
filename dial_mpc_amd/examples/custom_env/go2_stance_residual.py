"""Custom-environment example with a user control law: the Go2 of go2_height_walk (same reward, go2_height_walk.hip) driven by
residual control around its stance pose.  The law (go2_stance_residual.hip) maps an action to the home keyframe plus
action_scale x act x half the joint's sampling span and applies a PD torque on the actuator's own joint, so a zero action holds
the stance instead of the middle of the sampling range.  Both functions are compiled into one task plugin on first use.

    python -m dial_mpc_amd.core.dial_core --custom-env dial_mpc_amd.examples.custom_env.go2_stance_residual \\
        --config dial_mpc_amd/examples/custom_env/go2_stance_residual.yaml
"""
from dataclasses import dataclass

import numpy as np

from dial_mpc_amd.envs import register_config, register_environment
from dial_mpc_amd.examples.custom_env.go2_height_walk import Go2HeightWalkConfig, Go2HeightWalkEnv


@dataclass
class Go2StanceResidualConfig(Go2HeightWalkConfig):
    pass


class Go2StanceResidualEnv(Go2HeightWalkEnv):
    control_hip = "go2_stance_residual.hip"

    def task_dict(self):
        # the law reads the stance pose as the task's joint_offset (the home keyframe's joint angles)
        return dict(super().task_dict(), joint_offset=np.asarray(self._init_q[7:], dtype=np.float64))


register_config("go2_stance_residual", Go2StanceResidualConfig)
register_environment("go2_stance_residual", Go2StanceResidualEnv)
