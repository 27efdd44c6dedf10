"""Custom-environment example with a reference table: the Go2 tracks a periodic joint-space clip.  ``make_table`` generates the clip
-- 100 rows of 12 joint targets and a trunk height, one row per control step, no recorded data -- and the reward
(go2_track_clip.hip) reads the row of its control step through ``in.row``.  The table wraps around, so the clip repeats for as long as
the task runs; the state's step counter picks the row, in rollouts (step k of a rollout from step s0 looks ahead to row s0 + k) as in
env.step.

    python -m dial_mpc_amd.core.dial_core --custom-env dial_mpc_amd.examples.custom_env.go2_track_clip \\
        --config dial_mpc_amd/examples/custom_env/go2_track_clip.yaml
"""
from dataclasses import dataclass

import numpy as np

from dial_mpc_amd.envs import register_config, register_environment
from dial_mpc_amd.envs.custom_env import CustomEnv
from dial_mpc_amd.envs.unitree_go2_env import UnitreeGo2EnvConfig

CLIP_ROWS, CLIP_COLS = 100, 13   # one period of the clip; 12 joint targets | trunk height


@dataclass
class Go2TrackClipConfig(UnitreeGo2EnvConfig):
    w_joint: float = 1.0
    w_height: float = 10.0
    w_upright: float = 1.0
    w_ctrl: float = 1e-5
    clip_amp: float = 0.15       # [rad] amplitude of the thigh joints' swing; the calves move twice as far the other way
    clip_bob: float = 0.02       # [m] amplitude of the trunk's bobbing
    clip_height: float = 0.27    # [m] mean trunk height


class Go2TrackClipEnv(CustomEnv):
    model_path = "../../models/unitree_go2/mjx_scene_force.json"
    reward_hip = "go2_track_clip.hip"
    user_params = ("w_joint", "w_height", "w_upright", "w_ctrl")
    table_mode = "wrap"

    def __init__(self, config: Go2TrackClipConfig):
        super().__init__(config)
        self.joint_range = np.array(  # the walking envs' sampling range (unitree_go2_env.py)
            [[-0.5, 0.5], [0.4, 1.4], [-2.3, -0.85],
             [-0.5, 0.5], [0.4, 1.4], [-2.3, -0.85],
             [-0.5, 0.5], [0.4, 1.4], [-2.3, -1.3],
             [-0.5, 0.5], [0.4, 1.4], [-2.3, -1.3]])

    def make_table(self) -> np.ndarray:
        """One period of the clip, [CLIP_ROWS, CLIP_COLS]: the four legs squat and stretch around the home pose, diagonal pairs in
        antiphase (a trot in place without lifting a foot), and the trunk bobs at twice that rate.  Row r is phase 2 pi r / CLIP_ROWS,
        so the last row is followed by the first without a jump."""
        cfg = self._config
        home = np.asarray(self._init_q, dtype=np.float64)[7:19]
        phase = 2.0 * np.pi * np.arange(CLIP_ROWS) / CLIP_ROWS
        table = np.empty((CLIP_ROWS, CLIP_COLS), np.float64)
        table[:, :12] = home
        for leg, sign in enumerate((1.0, -1.0, -1.0, 1.0)):   # FR, FL, RR, RL: the diagonal pairs move together
            swing = sign * float(cfg.clip_amp) * np.sin(phase)
            table[:, 3 * leg + 1] += swing
            table[:, 3 * leg + 2] -= 2.0 * swing
        table[:, 12] = float(cfg.clip_height) + float(cfg.clip_bob) * np.cos(2.0 * phase)
        return table.astype(np.float32)


register_config("go2_track_clip", Go2TrackClipConfig)
register_environment("go2_track_clip", Go2TrackClipEnv)
