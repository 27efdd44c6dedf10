"""Inputs shared by tests/test_go2_unread_work_emu.py (host emulator) and tests/test_gpu_go2_unread_work.py (device)."""
import numpy as np

import smooth_ref as S
from conftest import perturbed_state, setup_case
from dial_mpc_amd import _abi
from dial_mpc_amd.core import spline

EX = "unitree_go2_trot"


def setup(N, H):
    """setup_case for the Go2 trot -- also at H = 1 (T = 2, the smallest rollout the reward stash allows), which make_cfg cannot
    configure: u2node (cfg.V, the map of dial_shift alone; no rollout reads it) is a quadratic spline through the T control steps
    and needs three.  There the cfg is filled here, with node2u (cfg.W) as ever and V = 0."""
    if H >= 2:
        return setup_case(EX, N, H)
    dc, env, model, task, _ = setup_case(EX, N, 2)
    dc.Hsample = H
    cfg = _abi.fill(_abi.DialCfg(), dict(Nsample=N, Hsample=H, Hnode=dc.Hnode, temp_sample=dc.temp_sample,
                                         W=spline.node2u_matrix(H, dc.Hnode), V=np.zeros((dc.Hnode + 1, H + 1))))
    return dc, env, model, task, cfg


def start_states(env, model, o32):
    """the rest pose (feet on the floor: the solver reaches its cap), a perturbed state, and a state in the air (smooth_ref.py class F,
    selected with the fp64 oracle: no active row, the solver stops by tolerance with niter = 0)"""
    q, qd = perturbed_state(env, 1)
    qa, va, _ = S.smooth_states(env, model, "F", 1, seed=17)
    return dict(rest=o32.env_reset(env._init_q, np.zeros(model.nv))[0], perturbed=o32.env_reset(q, qd)[0],
                air=o32.env_reset(qa[0], va[0])[0])
