"""The rollout gate of tests/smooth_ref.py on the host wave emulator (tests/emu_lib.py: the kernel body compiled for the CPU): five
env steps from class-F states against the fp64 oracle at rounding level, per step index, with no case left out.  Path 0 is the
dimension-specialised instantiation a model matches, path 1 the capacity-dimension one."""
import numpy as np
import pytest

import smooth_ref as S
from emu_lib import Emu

STATES, B = 4, 4
CASES = [(ex, 0) for ex in S.EXAMPLES] + [("unitree_go2_trot", 1), ("unitree_h1_loco", 1)]


@pytest.mark.parametrize("example,path", CASES, ids=[f"{ex}-path{p}" for ex, p in CASES])
def test_emulator_rollouts_at_rounding_level(example, path):
    _, env, model, task, cfg = S.case(example)
    o64, o32 = S.oracles(example)
    q, v, us = S.rollout_cases(example)
    us = np.ascontiguousarray(us[:STATES, :B])
    emu = Emu(model, task, cfg, path=path)
    resets = np.array([emu.env_reset(q[i], v[i], check_races=(i == 0))[0] for i in range(STATES)])
    gate = S.Gate(example, "F", "rollout", f"emulator-path{path}")
    gate.reset_blocks(model, o64, o32, q[:STATES], v[:STATES], resets)
    states = S.with_steps(resets)
    for i in range(STATES):   # from the emulator's own start state too, every physics step of the fp64 trajectories is in class F
        S.assert_stays_free(model, task, o64, states[i], us[i])
    got = [emu.rollout(states[i], us[i], check_races=(i == 0))[:4] for i in range(STATES)]
    got = tuple(np.stack([g[k] for g in got]) for k in range(4))
    r64, r32 = S.rollout_refs(o64, o32, states, us)
    gate.rollout_blocks(model, got, r64, r32)
    gate.check()
