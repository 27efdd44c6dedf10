"""The plugin model matrix without a GPU (tests/plugin_cases.py): the probe reward cross-compiles for every model of the matrix
(hipcc rejects no dimension combination, zero contacts / limits / sites included), the derived models have the dimensions they
claim, and a custom torque-mode model that the PD law's joint indexing does not fit is refused."""
import numpy as np
import pytest

from plugin_cases import CASES, build_matrix, case_model_dict


def test_probe_matrix_cross_compiles():
    from dial_mpc_amd.plugin import plugin_dims
    paths = build_matrix()
    assert set(paths) == set(CASES)
    dims = {n: plugin_dims(case_model_dict(n)) for n in CASES}
    assert paths["go2_nf4"] == paths["go2"]                 # n_frames is task data: one plugin
    assert len({paths[n] for n in CASES}) == len(CASES) - 1
    assert dims["go2_3con"]["ncon"] == 3
    assert dims["go2_free"]["ncon"] == 0 and dims["go2_free"]["nlim"] == 0 and case_model_dict("go2_free")["nefc"] == 0
    assert dims["go2_nosite"]["nsite"] == 0
    assert dims["h1_push_crate"]["nfri"] == 1 and dims["go2_crate"]["ncon"] == 52


def test_derived_models_have_the_constraint_rows_they_claim():
    """Each shipped model's nefc is its limit rows + dry-friction rows + 2 (condim - 1) pyramid rows per contact (the rule the derived
    models are built with); the derived Go2 models then hold the shipped Go2's rows minus what they drop -- 4 per contact (condim
    3), 1 per limit -- counted from the shipped model, not from that rule."""
    for n in ("go2", "go2_crate", "h1_walk", "h1_loco", "h1_push_crate"):
        m = case_model_dict(n)
        rows = int(m["nlim"]) + int(m.get("nfri", 0)) + int(sum(2 * (int(d) - 1) for d in np.asarray(m["con_dim"]).ravel()))
        assert int(m["nefc"]) == rows, n
    go2 = case_model_dict("go2")
    assert np.all(np.asarray(go2["con_dim"]) == 3) and int(go2["nfri"]) == 0
    assert case_model_dict("go2_3con")["nefc"] == int(go2["nefc"]) - 4
    assert case_model_dict("go2_free")["nefc"] == int(go2["nefc"]) - 4 * int(go2["ncon"]) - int(go2["nlim"]) == 0
    assert case_model_dict("go2_nosite")["nefc"] == int(go2["nefc"])


def test_multi_frame_case_runs_several_physics_steps_per_control_step():
    """go2_nf4 is the Go2 plugin's model at timestep 0.005 s under dt 0.02 s: 4 physics sub-steps per control step, in the task of the
    plugin context and of the oracle alike (were the override lost, its n_frames > 1 checks would quietly test n_frames == 1)."""
    from plugin_cases import load_case
    c = load_case("go2_nf4")
    assert c["otask"].n_frames == 4 and c["ptask"].n_frames == 4
    assert abs(c["model"].timestep - 0.005) < 1e-9 and abs(c["ptask"].dt - 0.02) < 1e-7
    assert load_case("go2")["otask"].n_frames == 1


def _permuted_go2_env(leg_control):
    from dial_mpc_amd.envs.custom_env import CustomEnv
    from dial_mpc_amd.envs.unitree_go2_env import UnitreeGo2EnvConfig

    class Permuted(CustomEnv):
        model_path = "../dial_mpc_amd/models/unitree_go2/mjx_scene_force.json"
        reward_hip = "plugin_probe.hip"

        def make_system(self, config):
            sys_ = super().make_system(config)
            m = sys_.model
            perm = np.r_[3:12, 0:3]                             # the front-right leg's three actuators moved to the end
            for k in [k for k in m if k.startswith("act_")]:
                m[k] = np.asarray(m[k])[perm]
            return sys_

    return Permuted(UnitreeGo2EnvConfig(leg_control=leg_control))


def test_torque_control_refuses_actuators_off_the_joint_convention():
    """Torque control indexes actuator a's joint as qpos[7 + a] / qvel[6 + a] (BaseEnv.act2tau, every kernel, the oracle); the
    force goes to act_qposadr / act_dofadr.  A Go2 whose actuators are permuted would get torques from the wrong joints, and the
    oracle makes the same mistake -- so CustomEnv refuses it under torque control, naming the convention, and accepts it under
    position control (which drives each actuator's own joint)."""
    with pytest.raises(ValueError, match=r"qpos\[7 \+ a\] / qvel\[6 \+ a\].*actuator 0 drives qpos 10 / dof 9"):
        _permuted_go2_env("torque")
    env = _permuted_go2_env("position")
    assert list(np.asarray(env.sys.model["act_qposadr"])[:3]) == [10, 11, 12]


def test_torque_convention_accepts_the_shipped_models():
    from dial_mpc_amd.envs.custom_env import torque_joint_convention
    for n in ("go2", "go2_crate", "h1_walk", "h1_loco", "h1_push_crate", "go2_free", "go2_nosite"):
        torque_joint_convention(case_model_dict(n))
