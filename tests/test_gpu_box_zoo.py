"""The box zoo of tests/box_zoo_cases.py on the device: per model a task plugin with the probe reward of tests/plugin_probe.hip (and the
capacity-dimension kernel under the Go2 walk task for box_pair), through what sits between a model and the box narrow phases --
box_of's pose composition, the compiler's con_sub order, the box-box polygon slices carved out of the dead velocity temporaries
(box_pair fills them exactly), the overflow copy of the constraint code and the compaction of touching contacts.

  in the air   test_gpu_synthetic_models._in_the_air, unchanged (smooth_ref's rule)
  in contact   test_gpu_synthetic_models._in_contact per start state of box_zoo_cases.contact_cases: 16 rollouts x 8 steps at
               conftest.TOL from the device's traced state, no unwitnessed transition, witnessed share <= 10 %; first the fp32 oracle
               against itself under 1 ulp of jitter (<= 5 %)
  geometry     one env_step_batch per model (n_frames = 1), one row per probed word of cdist / cpos in 32 states, against the fp64
               oracle's forward_dump of the same fp32 state at 8 x the fp32 oracle's own error per kind (floor 1e-6)
  bit identity con_cap = 1 (every touching step on the overflow area) == the default cap
  refusal      dial_create_plugin on box_pair_short

Each test prints its figures (SMOOTH / CHAIN / CONTACT / GEOMETRY lines); DESIGN.md section 2 records them."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import box_zoo_cases as B
import synthetic_cases as Z
from conftest import TOL, _within
from dial_mpc_amd import _abi
from plugin_cases import F
from test_gpu_synthetic_models import _dev, _host, _in_contact, _in_the_air, _step_chain, _walk_ctx

pytestmark = pytest.mark.gpu

K = _abi.MACROS
IU, IREW = K["DIAL_INFO_USER"], K["DIAL_INFO_REWARD"]


@pytest.fixture(scope="module")
def plugins(tmp_path_factory):
    """The probe plugin of every model, built once (or found in the cache), and box_pair_short's: build_plugin refuses that model
    (asserted), so its plugin is compiled with check_model out of the way -- what a user gets who builds a plugin another way."""
    from dial_mpc_amd import _lib, mjcf, plugin
    short = mjcf.compile_mjcf(B.box_pair_short(tmp_path_factory.mktemp("short")))
    with pytest.raises(_lib.DialHipError, match="4 box-box candidate contacts"):
        plugin.build_plugin(short, B.PROBE)
    mds = [B.load(n)["md"] for n in B.MODELS] + [short]
    real = plugin.check_model
    plugin.check_model = lambda m: None
    try:
        with ThreadPoolExecutor(max_workers=4) as ex:
            paths = list(ex.map(lambda md: plugin.build_plugin(md, B.PROBE), mds))
    finally:
        plugin.check_model = real
    out = dict(zip(B.MODELS + ("box_pair_short",), paths))
    out["box_pair_short_md"] = short
    return out


def _ctx(c, path, **opts):
    from dial_mpc_amd import _lib
    return _lib.Context(c["model"], c["ptask"], c["cfg"], device=0, plugin=path, user_params=list(B.PARAMS), options=opts)


# ------------------------------------------------------------------------------------------------------------------ in the air
@pytest.mark.parametrize("name", B.MODELS)
def test_plugin_in_the_air_at_rounding_level(plugins, name):
    c = B.load(name)
    _in_the_air(c, _ctx(c, plugins[name]), "plugin", rewards=False, mirror=False)


def test_capacity_kernel_in_the_air_on_box_pair():
    """box_pair without a plugin: the capacity-dimension kernel under the Go2 walk task, rewards gated."""
    c = B.load("box_pair")
    ctx = _walk_ctx(c)
    _in_the_air(c, ctx, "capacity-kernel", rewards=True, mirror=False)
    assert ctx.debug_last_launch()["inst"] == 0


# ------------------------------------------------------------------------------------------------------------------ in contact
def _reference_share(c, q, v, us):
    """The fp32 oracle against itself under 1 ulp of jitter through the same gate: witnessed / transitions over the start states."""
    model = c["model"]
    ni = model.nq + 2 * model.nv
    _, o32 = Z.oracles(c)
    tot = [0, 0]
    for i in range(len(q)):
        s0 = o32.env_reset(q[i], v[i])[0]
        ref = Z.contact_gate(c, o32, s0, us[i], *Z.jittered_oracle_run(o32, s0, us[i], ni, seed=5 + i), physics_only=False)
        assert not ref["unwitnessed"], ref["unwitnessed"]
        tot[0] += ref["witnessed"]
        tot[1] += ref["transitions"]
    return tot


def _box_kinds_touch(c, q, v):
    touch = B.touching_kinds(c, q, v)
    for k in B.BOX_KINDS:
        if k in np.asarray(c["md"]["con_kind"]).tolist():
            assert any(t[k] > 0 for t in touch), (c["name"], B.KIND_NAME[k], touch)


# Measured on one MI355X: DESIGN.md section 2, "Box contacts on synthetic robots".
@pytest.mark.parametrize("name", B.MODELS)
def test_plugin_in_contact_per_transition(plugins, name):
    """The start states put box features to work (box_zoo_cases.contact_cases says which); every box kind of the model has a slot with
    con_dist < 0 in one of them by the fp64 oracle."""
    c, q, v, us, labels = B.contact_cases(name)
    _box_kinds_touch(c, q, v)
    ref = _reference_share(c, q, v, us)
    print(f"CONTACT {name} reference: fp32 oracle under 1 ulp witnessed {ref[0]} / {ref[1]}")
    assert ref[0] <= Z.REFERENCE_CAP * ref[1], ref
    _in_contact(c, _ctx(c, plugins[name]), q, v, us, "plugin", physics_only=True, mirror=False)


def test_capacity_kernel_in_contact_on_box_pair():
    """box_pair on the capacity-dimension kernel: the same gate with the walk task's rewards.  Its workspace is carved at DimsMax, so
    the polygon slices have slack there; the refusal counts the model's own words all the same (dial_create)."""
    c, q, v, us, _ = B.contact_cases("box_pair")
    _in_contact(c, _walk_ctx(c), q, v, us, "capacity-kernel", physics_only=False, mirror=False)


# ------------------------------------------------------------------------------------------------------------------ contact geometry
@pytest.mark.parametrize("name", B.MODELS)
def test_contact_geometry_at_rounding_level(plugins, name):
    """cdist and cpos as the reward of the REAL kernel sees them, in the 32 geometry states: ONE env_step_batch launch with a row per
    (state, probed word), the selector in the row's info_user[0:2], n_frames = 1 (the reward's pre-integration inputs are the start
    state's).  box_zoo_cases.geometry_gate: per kind 8 x the fp32 oracle's own worst |fp32 - fp64| on the same slots (floor 1e-6),
    parked slots by test_gpu_plugin_matrix._check_parked, a live slot outside the tolerance needs an fp64 witness under <= 4 ulp of
    jitter on qpos, at most 1 % of the live slots witnessed."""
    c1 = B.load(name, frames=1)
    c, qs, vs = B.geometry_states(name)
    model = c1["model"]
    nq, nv, ncon = model.nq, model.nv, model.ncon
    ni = nq + 2 * nv
    ctx = _ctx(c1, plugins[name])
    s0, = _host(ctx.env_reset_batch(_dev(qs), _dev(vs)))
    assert np.array_equal(s0[:, nq:nq + nv], vs)
    s0[:, :nq] = qs          # (env.reset normalises the quaternions; the probed state is the fp32 state itself)
    words = [(F["cdist"], i) for i in range(ncon)] + [(F["cpos"], i) for i in range(3 * ncon)]
    S = np.repeat(s0, len(words), 0)
    S[:, ni + IU] = np.tile([f for f, _ in words], len(qs))
    S[:, ni + IU + 1] = np.tile([i for _, i in words], len(qs))
    out, = _host(ctx.env_step_batch(_dev(S), _dev(np.zeros((len(S), model.nu))))[0])
    ctx.status()
    rew = out[:, ni + IREW].reshape(len(qs), len(words))
    assert np.array_equal(out[:, :ni].reshape(len(qs), len(words), ni), np.repeat(out[::len(words), None, :ni], len(words), 1)), "rows differ in physics"
    B.assert_geometry(B.geometry_gate(name, rew[:, :ncon], rew[:, ncon:].reshape(len(qs), ncon, 3), "device"))


# ------------------------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("name", B.MODELS)
def test_overflow_area_is_bit_identical(plugins, name):
    """con_cap = 1: every step with more than one touching contact runs its constraint code on the overflow copy.  On every start state
    of the model's contact case: env.reset, the rollouts (rewards, q, qd, x) and the env.step chain equal the default cap's bit for
    bit; chain and rollout of the same actions both pass conftest.TOL against each other."""
    c, q, v, us, _ = B.contact_cases(name)
    model = c["model"]
    ctxs = [_ctx(c, plugins[name]), _ctx(c, plugins[name], con_cap=1)]
    for i in range(len(q)):
        res = []
        for ctx in ctxs:
            s0 = _host(ctx.env_reset_batch(_dev(q[i:i + 1]), _dev(v[i:i + 1])))[0][0]
            got = _host(*ctx.rollout(_dev(s0), _dev(us[i])))
            ctx.status()
            chain = _step_chain(ctx, model, s0, us[i, 0], mirror=False)
            for k, key in ((1, "q"), (2, "qd"), (3, "x")):
                assert _within(chain[k], got[k][0], TOL[key]).all(), (name, i, key, float(np.abs(chain[k] - got[k][0]).max()))
            res.append((s0, got, chain))
        assert ctxs[1].debug_last_launch()["con_cap"] == 1
        assert np.array_equal(res[0][0], res[1][0]), (name, i, "env.reset")
        for k in range(4):
            assert np.array_equal(res[0][1][k], res[1][1][k]), (name, i, "rollout", k)
            assert np.array_equal(res[0][2][k], res[1][2][k]), (name, i, "env.step chain", k)


# ------------------------------------------------------------------------------------------------------------------ refusal
def test_plugin_context_refuses_box_pair_short(plugins):
    """dial_create_plugin on box_pair_short with a plugin of its own dimensions: refused with DIAL_ERR_UNSUPPORTED and dial_create's
    message; on box_pair, the exact fit, the context comes to exist."""
    from dial_mpc_amd import _lib
    from conftest import LS_SWAP, with_solver
    c = B.load("box_pair")
    model = with_solver(_abi.make_model(plugins["box_pair_short_md"]), ls_rule=LS_SWAP)
    with pytest.raises(_lib.DialHipError, match="too many box-box candidate contacts for the polygon scratch") as e:
        _lib.Context(model, c["ptask"], c["cfg"], device=0, plugin=plugins["box_pair_short"], user_params=list(B.PARAMS))
    assert f"({K['DIAL_ERR_UNSUPPORTED']})" in str(e.value)
    _ctx(c, plugins["box_pair"])
