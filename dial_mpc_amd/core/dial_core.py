"""``MBDPI`` -- the DIAL-MPC planner with the reference's Python surface (dial_mpc/core/dial_core.py:51-172)
on top of the HIP kernels, plus the synchronous-simulation driver ``main`` (dial_core.py:175-329).

Differences that are deliberate and documented:
* ``rng`` is a ``torch.Generator`` on the GPU (or an int seed) instead of a JAX key; the noise ``eps`` can
  also be passed explicitly (``eps=``) so that "identical noise draws" means *the same array*
  (JAX's threefry stream is version dependent).
* samples shard over the ranks of ``torch.distributed`` when it is initialised.
* the Brax HTML render / Flask server at the end of the reference's ``main`` are out of scope.
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import time
from typing import Any, Dict, Optional

import numpy as np

from dial_mpc_amd import _abi, _lib
from dial_mpc_amd.core import spline
from dial_mpc_amd.core.dial_config import DialConfig


def make_cfg(args: DialConfig) -> "_abi.DialCfg":
    W = spline.node2u_matrix(args.Hsample, args.Hnode)
    V = spline.u2node_matrix(args.Hsample, args.Hnode)
    return _abi.fill(_abi.DialCfg(), dict(Nsample=args.Nsample, Hsample=args.Hsample, Hnode=args.Hnode,
                                          temp_sample=args.temp_sample, W=W, V=V))


def softmax_update(weights, Y0s, sigma, mu_0t):
    """dial_core.py:45-48 (kept for API parity; the kernels compute the same einsum in K4b)."""
    import torch
    return torch.einsum("n,nij->ij", weights, Y0s), sigma


def elite_update(weights, Y0s, sigma, mu_0t):
    """The update of "cem" / "ps" (kept for API parity, like softmax_update): the same einsum over the elite weights -- 1 / K on the K
    best candidates, zero elsewhere (include/dial_mpc.h: DIAL_UPDATE_ELITE).  sigma passes through: the noise schedule stays DIAL's."""
    import torch
    return torch.einsum("n,nij->ij", weights, Y0s), sigma


UPDATE_FNS = {"mppi": softmax_update, "cem": elite_update, "ps": elite_update}


class MBDPI:
    def __init__(self, args: DialConfig, env, device: Optional[int] = None, kernel_rng: bool = False,
                 force_sharded: bool = False, options: Optional[dict] = None, n_plans: int = 1,
                 models=None, model_of=None, model_per: str = "plan", ensemble: Optional[dict] = None):
        """kernel_rng=True: the noise is generated inside the rollout kernel (Philox keyed by args.seed and a call
        counter) instead of by torch.randn -- the production setting; parity runs pass `eps` explicitly.
        force_sharded (measurement hook): run the sharded code path, collectives included, on a 1-rank process group.
        options: `dial_options` fields for the context (launch-shape / measurement switches, include/dial_mpc.h).
        n_plans: plans one reverse_once_batch call may carry (the context's dial_options.plan_cap).
        models / model_of / model_per: planner models bound at creation (set_models); a custom environment's context is then created on
        the plugin that carries the per-model rollout kernel (CustomEnv.plugin_path(plan_models=True)).
        ensemble: dict(models=, hyp=, aggregate=, alpha=) -- a model ensemble bound at creation (set_ensemble); a custom environment's
        context is then created on the plugin that carries the ensemble rollout kernel (plan_ensemble=True)."""
        import torch
        self.kernel_rng = bool(kernel_rng)
        self._rng_counter = 0
        self._last_plans, self._last_batched = 1, False   # shape of the last call's weights (weights())
        self._plan = None   # preallocated buffers of the sharded iteration (core/sharding.py)
        self._force_sharded = bool(force_sharded)
        self.args = args
        self.env = env
        self.nu = env.action_size
        self.update_fn = UPDATE_FNS[args.update_method]  # KeyError for anything else, as upstream
        if args.update_method != "mppi":   # (refuse a bad elite set before anything is created)
            _lib.elite_count(args.update_method, args.Nsample, getattr(args, "elite_frac", 0.1), getattr(args, "n_elite", 0))

        sigma_control = args.horizon_diffuse_factor ** np.arange(args.Hnode + 1)[::-1]  # dial_core.py:66-70
        sigma_control = sigma_control * args.sigma_scale
        self.ctrl_dt = 0.02  # hard-coded upstream (dial_core.py:74)
        self.step_us_np = np.linspace(0, self.ctrl_dt * args.Hsample, args.Hsample + 1)
        self.step_nodes_np = np.linspace(0, self.ctrl_dt * args.Hsample, args.Hnode + 1)
        self.node_dt = self.ctrl_dt * args.Hsample / args.Hnode

        self.cfg = make_cfg(args)
        # sample sharding over torch.distributed ranks (one process per GPU)
        self.rank, self.world = 0, 1
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                self.rank, self.world = dist.get_rank(), dist.get_world_size()
        except Exception:
            pass
        from dial_mpc_amd.core.sharding import partition
        self._per, self.n_begin, self.n_local = partition(args.Nsample, self.rank, self.world)
        if int(n_plans) < 1:
            raise ValueError("n_plans must be >= 1")
        self.n_plans = int(n_plans)
        if self.n_plans > 1:
            options = dict(options or {}, plan_cap=self.n_plans)
        # a rank's rollout scratch is sized by its own shard, not by the global sample count
        extra = {}
        if hasattr(env, "context_kwargs"):   # (custom envs: their task plugin, envs/custom_env.py)
            if models is not None and ensemble is not None:
                raise ValueError("MBDPI: models= (set_models) and ensemble= (set_ensemble) exclude each other")
            if ensemble is not None:
                extra = env.context_kwargs(plan_ensemble=True)
            else:
                extra = env.context_kwargs(plan_models=True) if models is not None else env.context_kwargs()
        self.ctx = _lib.Context(env.make_model(), env.make_task(), self.cfg, device,
                                n_local_cap=None if self.world == 1 else self._per, options=options, **extra)
        if hasattr(env, "bind_device"):
            env.bind_device(self.ctx.device)
        dev = self.ctx.torch_device
        self.device = dev
        self.sigma_control = torch.as_tensor(sigma_control.copy(), dtype=torch.float32, device=dev)
        self.step_us = torch.as_tensor(self.step_us_np, dtype=torch.float32, device=dev)
        self.step_nodes = torch.as_tensor(self.step_nodes_np, dtype=torch.float32, device=dev)
        self.W = torch.as_tensor(spline.node2u_matrix(args.Hsample, args.Hnode), dtype=torch.float32, device=dev)
        self.V = torch.as_tensor(spline.u2node_matrix(args.Hsample, args.Hnode), dtype=torch.float32, device=dev)
        self.update_method, self.n_elite = "mppi", 0
        if args.update_method != "mppi":   # (on every rank of a sharded run: each forms the global weights itself)
            self.set_update(args.update_method)
        self.model_of = None
        if models is not None:
            self.set_models(models, model_of, model_per)
        self.hyp = None
        if ensemble is not None:
            unknown = sorted(set(ensemble) - {"models", "hyp", "aggregate", "alpha"})
            if unknown or "models" not in ensemble:
                raise ValueError(f"MBDPI: ensemble is dict(models=, hyp=, aggregate=, alpha=); got keys {sorted(ensemble)}")
            self.set_ensemble(**ensemble)

    # ---- update rules (dial_set_update_rule; csrc/update_rule.h)
    def set_update(self, method: str, elite_frac: Optional[float] = None, n_elite: Optional[int] = None):
        """Rebind the rule that turns rewards into weights; the calls issued afterwards use it.  method: "mppi" (softmax), "cem"
        (uniform weights on the K best candidates, K = n_elite or ceil(elite_frac Nsample)) or "ps" (K = 1: the plan becomes the best
        candidate); KeyError for anything else.  elite_frac / n_elite None: the config's.  self.args is left as it is; self.update_method
        and self.n_elite name what is bound.  The sampling noise is not adapted from the elites.  In a sharded run every rank makes the
        same call.  Returns K (0 for mppi)."""
        fn = UPDATE_FNS[method]
        frac = getattr(self.args, "elite_frac", 0.1) if elite_frac is None else elite_frac
        ne = getattr(self.args, "n_elite", 0) if n_elite is None else n_elite
        K = 0 if method == "mppi" else _lib.elite_count(method, self.args.Nsample, frac, ne)
        self.ctx.set_update_rule("mppi" if K == 0 else "elite", K)
        self.update_fn, self.update_method, self.n_elite = fn, method, K
        return K

    def weights(self):
        """The weights the last reverse_once [N + 1] or reverse_once_batch [M, N + 1] formed (the softmax weights under mppi too), e.g.
        for an effective sample size 1 / sum(w^2).  A sharded run returns the global weights, the same on every rank."""
        w = self.ctx.weights(self._last_plans)
        return w if self._last_batched else w[0]

    # ---- robust planning over a model ensemble (dial_set_plan_ensemble; csrc/plan_ens_kernel.h)
    def set_ensemble(self, models, hyp=None, aggregate: str = "mean", alpha: float = 1.0):
        """Bind a model ensemble: `models` a list of V compiled model dicts (mjcf.vary_model(env.sys.model, ...)), `hyp` the
        hypotheses -- [R] indices shared by all plans, or [n_plans][R]; None: all V models in order.  Every candidate of
        reverse_once / reverse_once_batch is then rolled out under all R hypotheses of its plan and weighted by the aggregate of its R
        rewards: "mean", "min", or "cvar" (the mean of the ceil(alpha R) worst).  The bars are the weighted means of the trajectories
        under hypothesis 0, the plan's nominal model.  Every dict gets the env's timestep; env.step and the plant keep their own
        model.  models None unbinds.  Returns the hypotheses bound."""
        if models is None:
            self.ctx.set_plan_ensemble(None)
            self.hyp = None
            return None
        if self.world > 1 or self._force_sharded:
            raise NotImplementedError("set_ensemble: model ensembles run on one rank (sharded contexts are not supported)")
        dt = float(self.env.make_model().timestep)
        structs = []
        for m in models:
            st = _abi.make_model(m)
            st.timestep = dt
            structs.append(st)
        index = _lib.plan_ensemble_index(hyp, len(structs), self.n_plans)
        self.hyp = self.ctx.set_plan_ensemble(structs, index, aggregate, alpha)
        return self.hyp

    # ---- planner model ensembles (dial_set_plan_models; csrc/plan_var_kernel.h)
    def set_models(self, models, model_of=None, per: str = "plan"):
        """Bind planner models: `models` a list of V compiled model dicts (mjcf.vary_model(env.sys.model, ...)).  per="plan": plan g of
        reverse_once_batch plans with models[model_of[g]] (`model_of` [n_plans]; None: g % V), reverse_once with models[model_of[0]].
        per="sample": rollout n of every plan runs models[model_of[n]] (`model_of` [Nsample + 1], the mean trajectory last; None:
        n % V, the mean trajectory model 0) -- domain-randomised sampling.  Every dict gets the env's timestep.  env.step and the
        plant keep their own model.  models None unbinds.  Returns the index bound."""
        if models is None:
            self.ctx.set_plan_models(None)
            self.model_of = None
            return None
        if self.world > 1 or self._force_sharded:
            raise NotImplementedError("set_models: planner models run on one rank (sharded contexts are not supported)")
        dt = float(self.env.make_model().timestep)
        structs = []
        for m in models:
            st = _abi.make_model(m)
            st.timestep = dt
            structs.append(st)
        rows = self.args.Nsample + 1 if per == "sample" else self.n_plans
        index = _lib.plan_model_index(model_of, len(structs), rows, per)
        self.model_of = self.ctx.set_plan_models(structs, index, per)
        return self.model_of

    # ---- spline maps (constant matrices; dial_core.py:82-101)
    def node2u(self, nodes):
        return self.W @ nodes

    def u2node(self, us):
        return self.V @ us

    def node2u_vmap(self, Y):          # (Hnode+1, nu) -> (Hsample+1, nu)
        return self.W @ Y

    def u2node_vmap(self, u):
        return self.V @ u

    def node2u_vvmap(self, Ys):        # (B, Hnode+1, nu) -> (B, Hsample+1, nu)
        import torch
        return torch.einsum("tk,bka->bta", self.W, Ys)

    def u2node_vvmap(self, us):
        import torch
        return torch.einsum("kt,bta->bka", self.V, us)

    def rollout_us(self, state, us):
        rewss, qss, qdss, xss = self.ctx.rollout(_packed(state), us[None].contiguous())
        return rewss[0], dict(q=qss[0], qd=qdss[0], x_pos=xss[0].reshape(us.shape[0], -1, 3))

    def rollout_us_vmap(self, state, us):
        rewss, qss, qdss, xss = self.ctx.rollout(_packed(state), us.contiguous())
        B, T = us.shape[:2]
        return rewss, dict(q=qss, qd=qdss, x_pos=xss.reshape(B, T, -1, 3))

    # ---- one annealing iteration (dial_core.py:103-145)
    def sample_eps(self, rng):
        import torch
        gen = _generator(rng, self.device)
        eps = torch.randn((self.args.Nsample, self.args.Hnode + 1, self.nu), generator=gen, device=self.device,
                          dtype=torch.float32)
        return gen, eps

    def reverse_once(self, state, rng, Ybar_i, noise_scale, eps=None, want_bars: bool = True):
        """want_bars=False skips qbar/qdbar/xbar (None in info): the rollouts then do not write their per-step states and K4b
        sums the candidate nodes only; in a sharded run this also drops the all-reduce, leaving one collective per annealing
        iteration (core/sharding.py).  The drivers ask for the bars on the last iteration of a plan only, as upstream reads
        them (dial_core.py:262-264, dial_plan.py:214-215)."""
        import torch
        packed = _packed(state)
        self._last_plans, self._last_batched = 1, False
        if eps is None and self.kernel_rng:
            Yb = torch.as_tensor(Ybar_i, dtype=torch.float32, device=self.device).contiguous()
            nsc = torch.as_tensor(noise_scale, dtype=torch.float32, device=self.device).reshape(-1).contiguous()
            T, nb1 = self.args.Hsample + 1, self.ctx.nbody - 1
            counter = self._rng_counter
            self._rng_counter += 1
            if self.world == 1 and not self._force_sharded:
                out = self.ctx.reverse_once_rng(packed, Yb, nsc, int(self.args.seed), counter, want_bars=want_bars)
                Ybar, rews, qbar, qdbar, xbar = out["Ybar"], out["rews"], out["qbar"], out["qdbar"], out["xbar"]
            else:   # sharded: every rank draws its own shard's noise (and, for the mean action, everybody's) in-kernel
                Ybar, rews, qbar, qdbar, xbar = self._reverse_once_sharded(packed, Yb, nsc, None, want_bars,
                                                                           rng=(int(self.args.seed), counter))
            return rng, Ybar, {"rews": rews, "qbar": qbar, "qdbar": qdbar,
                               "xbar": xbar.reshape(T, nb1, 3) if xbar is not None else None, "new_noise_scale": nsc}
        if eps is None:
            rng, eps = self.sample_eps(rng)
        Ybar_i = torch.as_tensor(Ybar_i, dtype=torch.float32, device=self.device).contiguous()
        noise_scale = torch.as_tensor(noise_scale, dtype=torch.float32, device=self.device).reshape(-1).contiguous()
        T, nb1 = self.args.Hsample + 1, self.ctx.nbody - 1
        if self.world == 1 and not self._force_sharded:
            out = self.ctx.reverse_once(packed, Ybar_i, noise_scale, eps.contiguous(), want_bars=want_bars)
            Ybar, rews = out["Ybar"], out["rews"]
            qbar, qdbar, xbar = out["qbar"], out["qdbar"], out["xbar"]
        else:
            Ybar, rews, qbar, qdbar, xbar = self._reverse_once_sharded(packed, Ybar_i, noise_scale, eps, want_bars)
        info = {"rews": rews, "qbar": qbar, "qdbar": qdbar, "xbar": xbar.reshape(T, nb1, 3) if xbar is not None else None,
                "new_noise_scale": noise_scale}
        return rng, Ybar, info

    def _reverse_once_sharded(self, packed, Ybar_i, noise_scale, eps, want_bars=True, rng=None):
        import torch.distributed as dist
        from dial_mpc_amd.core.sharding import ShardPlan, sharded_reverse_once
        if self._plan is None:
            self._plan = ShardPlan(self.ctx, self.rank, self.world, self.args.Nsample, self.args.Hsample + 1,
                                   self.args.Hnode + 1)
        return sharded_reverse_once(self.ctx, dist, self.rank, self.world, self.args.Nsample, self.args.Hsample + 1,
                                    self.args.Hnode + 1, packed, Ybar_i, noise_scale,
                                    eps.contiguous() if eps is not None else None, want_bars, plan=self._plan, rng=rng)

    # ---- M independent plans in one launch: jax.vmap(reverse_once) over (state, rng, Ybar_i, noise_scale)
    def reverse_once_batch(self, states, rng, Ybars, noise_scales, eps=None, want_bars: bool = True, user_params=None):
        """states: list of M States or packed [M, state_size]; Ybars [M, Hnode+1, nu]; noise_scales [M, ns] (or [ns]: the same for all).
        eps [M, N, Hnode+1, nu] explicit noise; None: kernel_rng -> in-kernel Philox (plan g draws global samples g N ..), else
        torch.randn from `rng`.  user_params: per-plan task parameters [M, n] of a custom environment (CustomEnv.plan_params), plan g's
        reward reads row g -- bound on this planner's context for this call only.  Returns (rng, Ybar [M, Hnode+1, nu], info) with
        info rews [M, N+1], qbar / qdbar [M, T, .], xbar [M, T, nbody-1, 3] (None with want_bars=False) and new_noise_scale."""
        import torch
        if self.world > 1 or self._force_sharded:
            raise NotImplementedError("reverse_once_batch: grouped plans run on one rank (sharded batches are not supported)")
        if user_params is not None:
            if self.ctx.plugin is None:
                raise ValueError("reverse_once_batch: per-plan task parameters (user_params=) need a custom environment's task plugin")
            self.ctx.set_plan_params(user_params)
            try:
                return self.reverse_once_batch(states, rng, Ybars, noise_scales, eps=eps, want_bars=want_bars)
            finally:
                self.ctx.set_plan_params(None)
        if isinstance(states, (list, tuple)):
            states = torch.stack([_packed(st) for st in states])
        states = torch.as_tensor(states, dtype=torch.float32, device=self.device).contiguous()
        M = int(states.shape[0])
        self._last_plans, self._last_batched = M, True
        Ybars = torch.as_tensor(Ybars, dtype=torch.float32, device=self.device).contiguous()
        nsc = torch.as_tensor(noise_scales, dtype=torch.float32, device=self.device)
        if nsc.dim() < 2:
            nsc = nsc.reshape(1, -1).expand(M, -1)
        nsc = nsc.reshape(M, -1).contiguous()
        T, nb1 = self.args.Hsample + 1, self.ctx.nbody - 1
        if eps is None and self.kernel_rng:
            counter = self._rng_counter
            self._rng_counter += 1
            out = self.ctx.reverse_once_batch_rng(states, Ybars, nsc, int(self.args.seed), counter, want_bars=want_bars)
        else:
            if eps is None:
                gen = _generator(rng, self.device)
                eps = torch.randn((M, self.args.Nsample, self.args.Hnode + 1, self.nu), generator=gen, device=self.device,
                                  dtype=torch.float32)
                rng = gen
            out = self.ctx.reverse_once_batch(states, Ybars, nsc, eps.contiguous(), want_bars=want_bars)
        xbar = out["xbar"]
        info = {"rews": out["rews"], "qbar": out["qbar"], "qdbar": out["qdbar"],
                "xbar": xbar.reshape(M, T, nb1, 3) if xbar is not None else None, "new_noise_scale": nsc}
        return rng, out["Ybar"], info

    def shift_batch(self, Ys):
        """shift of M plans in one launch: Ys [M, Hnode+1, nu]."""
        import torch
        Ys = torch.as_tensor(Ys, dtype=torch.float32, device=self.device).contiguous()
        return self.ctx.shift_batch(Ys)

    # ---- receding-horizon shift (dial_core.py:160-172)
    def shift(self, Y):
        import torch
        Y = torch.as_tensor(Y, dtype=torch.float32, device=self.device).contiguous()
        return self.ctx.shift(Y)

    def shift_Y_from_u(self, u, n_step):
        import torch
        u = torch.roll(u, -n_step, dims=0)
        u[-n_step:] = 0
        return self.u2node_vmap(u)


def _packed(state):
    return state.packed if hasattr(state, "packed") else state


def _generator(rng, device):
    import torch
    if isinstance(rng, torch.Generator):
        return rng
    gen = torch.Generator(device=device)
    gen.manual_seed(int(rng) if rng is not None else 0)
    return gen


def load_dial_and_env(config_dict: Dict[str, Any]):
    import dial_mpc_amd.envs as dial_envs
    from dial_mpc_amd.utils.io_utils import load_dataclass_from_dict
    dial_config = load_dataclass_from_dict(DialConfig, config_dict)
    env_config_type = dial_envs.get_config(dial_config.env_name)
    env_config = load_dataclass_from_dict(env_config_type, config_dict, convert_list_to_array=True)
    env_config.seed = int(dial_config.seed)      # randomize_tasks draws from the run's seed (envs/base_env.py)
    env = dial_envs.get_environment(dial_config.env_name, config=env_config)
    return dial_config, env_config, env


_PLAN_MODEL_KEYS = ("per", "variants", "model_of")


def plan_models_settings(block: Dict[str, Any], model: Dict[str, Any], n_plans: int, Nsample: int):
    """A `plan_models` block of the driver's YAML -> (models, model_of, per) for MBDPI(models=, model_of=, model_per=):
        per: plan | sample            (default plan)
        variants: [ {...}, ... ]      each entry the keywords of mjcf.vary_model; {} is the env's model
        model_of: [...]               optional; n_plans entries per plan, Nsample + 1 per sample (the mean trajectory last)
    Raises ValueError on unknown keys, an empty variant list, whatever vary_model refuses and an index of the wrong length or range."""
    from dial_mpc_amd.deploy.dial_sim import sim_model_settings
    if not isinstance(block, dict):
        raise ValueError(f"plan_models is a mapping; got {type(block).__name__}")
    unknown = sorted(set(block) - set(_PLAN_MODEL_KEYS))
    if unknown:
        raise ValueError(f"plan_models: unknown keys {unknown}; known: {list(_PLAN_MODEL_KEYS)}")
    per = block.get("per", "plan")
    if per not in ("plan", "sample"):
        raise ValueError(f"plan_models: per = {per!r}; 'plan' or 'sample' are allowed")
    variants = block.get("variants")
    if not isinstance(variants, (list, tuple)) or len(variants) < 1:
        raise ValueError("plan_models: variants is a non-empty list of mjcf.vary_model keyword mappings ({} is the env's model)")
    models = []
    for v, entry in enumerate(variants):
        try:
            models.append(sim_model_settings({} if entry is None else entry, model))
        except ValueError as e:
            raise ValueError(f"plan_models: variant {v}: {str(e).replace('sim_model: ', '').replace('sim_model ', 'it ')}") from None
    rows = int(Nsample) + 1 if per == "sample" else int(n_plans)
    index = _lib.plan_model_index(block.get("model_of"), len(models), rows, per)
    return models, index, per


_PLAN_ENSEMBLE_KEYS = ("variants", "hypotheses", "aggregate", "alpha")


def plan_ensemble_settings(block: Dict[str, Any], model: Dict[str, Any], n_plans: int):
    """A `plan_ensemble` block of the driver's YAML -> dict(models=, hyp=, aggregate=, alpha=) for MBDPI(ensemble=):
        variants: [ {...}, ... ]      each entry the keywords of mjcf.vary_model; {} is the env's model
        hypotheses: [...]             optional; R indices shared by all plans, or one list of R per plan; default: all variants in order
        aggregate: mean | min | cvar  (default mean)
        alpha: 0.5                    cvar only: the tail's share, in (0, 1] (default 1)
    Raises ValueError on unknown keys, an empty variant list, whatever vary_model refuses, bad indices, an unknown aggregate and an
    alpha outside (0, 1]."""
    from dial_mpc_amd.deploy.dial_sim import sim_model_settings
    if not isinstance(block, dict):
        raise ValueError(f"plan_ensemble is a mapping; got {type(block).__name__}")
    unknown = sorted(set(block) - set(_PLAN_ENSEMBLE_KEYS))
    if unknown:
        raise ValueError(f"plan_ensemble: unknown keys {unknown}; known: {list(_PLAN_ENSEMBLE_KEYS)}")
    aggregate = block.get("aggregate", "mean")
    if aggregate not in _lib.ENSEMBLE_AGGREGATES:
        raise ValueError(f"plan_ensemble: aggregate = {aggregate!r}; {sorted(_lib.ENSEMBLE_AGGREGATES)} are allowed")
    alpha = block.get("alpha", 1.0)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"plan_ensemble: alpha = {alpha!r}; a number in (0, 1] is allowed")
    variants = block.get("variants")
    if not isinstance(variants, (list, tuple)) or len(variants) < 1:
        raise ValueError("plan_ensemble: variants is a non-empty list of mjcf.vary_model keyword mappings ({} is the env's model)")
    models = []
    for v, entry in enumerate(variants):
        try:
            models.append(sim_model_settings({} if entry is None else entry, model))
        except ValueError as e:
            raise ValueError(f"plan_ensemble: variant {v}: {str(e).replace('sim_model: ', '').replace('sim_model ', 'it ')}") from None
    try:
        hyp = _lib.plan_ensemble_index(block.get("hypotheses"), len(models), int(n_plans))
    except ValueError as e:
        raise ValueError(str(e).replace("plan ensemble: hyp", "plan_ensemble: hypotheses").replace("plan ensemble:", "plan_ensemble:")) from None
    return dict(models=models, hyp=hyp, aggregate=aggregate, alpha=float(alpha))


def _plan_models_kw(config_dict, dial_config, env, n_plans: int) -> Dict[str, Any]:
    """The MBDPI keywords of the YAML's optional plan_models or plan_ensemble block; {} when both are absent (nothing is bound)."""
    ens = config_dict.get("plan_ensemble")
    if ens is not None:
        if config_dict.get("plan_models") is not None:
            raise ValueError("plan_models and plan_ensemble exclude each other: keep one of the two blocks")
        kw = plan_ensemble_settings(ens, env.sys.model, n_plans)
        print(f"planner ensemble: {len(kw['models'])} variants, hypotheses of plan 0 = {kw['hyp'][0].tolist()}, aggregate = {kw['aggregate']}"
              + (f" (alpha = {kw['alpha']})" if kw["aggregate"] == "cvar" else ""))
        return dict(ensemble=kw)
    block = config_dict.get("plan_models")
    if block is None:
        return {}
    models, index, per = plan_models_settings(block, env.sys.model, n_plans, dial_config.Nsample)
    print(f"planner models: {len(models)} variants per {per}, model_of = {index.tolist() if index.size <= 32 else str(index[:32].tolist()) + ' ...'}")
    return dict(models=models, model_of=index, model_per=per)


def _positive_int(v: str) -> int:
    n = int(v)
    if n < 1:
        raise argparse.ArgumentTypeError(f"must be >= 1, got {v}")
    return n


def _env_params(parser, args, env):
    """--env-param NAME=V1,...,VM -> {NAME: [V1 .. VM]}, checked against the env and --n-envs before anything runs."""
    if not args.env_param:
        return None
    if not hasattr(env, "plan_params"):
        parser.error(f"--env-param: {type(env).__name__} is a built-in environment; per-loop task parameters need a custom environment")
    if args.n_envs < 2:
        parser.error("--env-param needs --n-envs M with M > 1 (one closed loop takes its parameters from the config)")
    out = {}
    for item in args.env_param:
        name, sep, vals = item.partition("=")
        name = name.strip()
        try:
            values = [float(v) for v in vals.split(",")] if sep and vals.strip() else None
        except ValueError:
            values = None
        if not name or values is None:
            parser.error(f"--env-param {item!r}: expected NAME=V1,...,VM")
        if name not in env.user_params:
            parser.error(f"--env-param: {name!r} is not one of the task parameters {list(env.user_params)}")
        if len(values) != args.n_envs:
            parser.error(f"--env-param {name}: {len(values)} values for --n-envs {args.n_envs}")
        if name in out:
            parser.error(f"--env-param {name} given twice")
        out[name] = values
    return out


def main(argv=None):
    """Synchronous simulation driver: the body of the reference's ``main`` (dial_core.py:175-329).
    ``--n-envs M`` (M > 1) runs M closed loops through the grouped entry points (main_batched)."""
    import torch
    import yaml
    from dial_mpc_amd.examples import examples
    from dial_mpc_amd.utils.io_utils import get_example_path

    parser = argparse.ArgumentParser()
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument("--config", type=str, default=None)
    group.add_argument("--example", type=str, default=None)
    group.add_argument("--list-examples", action="store_true")
    parser.add_argument("--custom-env", type=str, default=None, help="Custom environment to import dynamically")
    parser.add_argument("--n-steps", type=int, default=None, help="override n_steps from the YAML")
    parser.add_argument("--n-envs", type=_positive_int, default=1,
                        help="M closed loops from env.reset, planned together in one launch per iteration (default 1)")
    parser.add_argument("--env-param", action="append", default=[], metavar="NAME=V1,...,VM",
                        help="custom environments with --n-envs M: closed loop g runs with task parameter NAME = Vg (repeatable)")
    parser.add_argument("--update-method", choices=sorted(UPDATE_FNS), default=None,
                        help="override update_method from the YAML: mppi (softmax), cem (elite mean) or ps (best sample)")
    parser.add_argument("--elite-frac", type=float, default=None,
                        help="override elite_frac from the YAML: cem's elites as a share of Nsample, in (0, 1] (clears n_elite)")
    args = parser.parse_args(argv)

    if args.list_examples:
        print("Examples:")
        for example in examples:
            print(f"  {example}")
        return
    if args.custom_env is not None:
        sys.path.append(os.getcwd())
        importlib.import_module(args.custom_env)
    if args.example is not None:
        config_dict = yaml.safe_load(open(get_example_path(args.example + ".yaml")))
    else:
        config_dict = yaml.safe_load(open(args.config))
    dial_config, env_config, env = load_dial_and_env(config_dict)
    if args.n_steps is not None:
        dial_config.n_steps = args.n_steps
    if args.update_method is not None:
        dial_config.update_method = args.update_method
    if args.elite_frac is not None:
        dial_config.elite_frac, dial_config.n_elite = args.elite_frac, 0
    env_params = _env_params(parser, args, env)
    model_kw = _plan_models_kw(config_dict, dial_config, env, args.n_envs)
    if args.n_envs > 1:
        extra = dict(model_kw=model_kw) if model_kw else {}   # (absent block: the calls are the ones of before)
        if env_params:
            return main_batched(dial_config, env, args.n_envs, env_params=env_params, **extra)
        return main_batched(dial_config, env, args.n_envs, **extra)
    print("Creating environment")
    mbdpi = MBDPI(dial_config, env, **model_kw)
    rng = _generator(dial_config.seed, mbdpi.device)
    state = env.reset(rng)
    Y0 = torch.zeros((dial_config.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=mbdpi.device)

    rews, rews_plan, rollout, infos = [], [], [], []
    plan_ms = []
    for t in range(dial_config.n_steps):
        state = env.step(state, Y0[0])                      # dial_core.py:245
        rollout.append(state)
        rews.append(float(state.reward))
        Y0 = mbdpi.shift(Y0)                                # :251
        n_diffuse = dial_config.Ndiffuse_init if t == 0 else dial_config.Ndiffuse
        t0 = time.time()
        factors = mbdpi.sigma_control[None, :] * (dial_config.traj_diffuse_factor **
                                                  torch.arange(n_diffuse, device=mbdpi.device))[:, None]
        info = None
        for i in range(n_diffuse):                          # lax.scan(reverse_scan) :262-264
            rng, Y0, info = mbdpi.reverse_once(state, rng, Y0, factors[i], want_bars=(i == n_diffuse - 1))
        torch.cuda.synchronize()
        mbdpi.ctx.status()                                   # raises if an asynchronous launch of this tick gave up
        plan_ms.append((time.time() - t0) * 1e3)
        rews_plan.append(float(info["rews"].mean()))         # :266 mean over all N+1 sample rewards of the last iteration
        infos.append(info)
        if t % 20 == 0:
            print(f"step {t:4d}  rew {rews[-1]: .3e}  plan {plan_ms[-1]:.2f} ms")
    print(f"mean reward = {np.mean(rews):.2e}")
    if len(plan_ms) > 1:
        print(f"plan latency p50 = {np.percentile(plan_ms[1:], 50):.3f} ms (tick = 20 ms)")

    os.makedirs(dial_config.output_dir, exist_ok=True)
    timestamp = time.strftime("%Y%m%d-%H%M%S")
    states_arr, pred_arr = result_arrays(rollout, infos)
    np.save(os.path.join(dial_config.output_dir, f"{timestamp}_states"), states_arr)
    np.save(os.path.join(dial_config.output_dir, f"{timestamp}_predictions"), pred_arr)


def batched_loop(mbdpi: "MBDPI", env, states, n_steps: int, eps_fn=None, on_tick=None, user_params=None):
    """M closed loops of the synchronous driver, planned together: per tick env.step of all M states (one launch), shift of all M
    plans, then Ndiffuse grouped annealing iterations.  eps_fn(t, i) -> eps [M, N, Hnode+1, nu] or None (noise from the planner's rng
    / kernel_rng).  user_params: per-loop task parameters [M, n] of a custom environment (CustomEnv.plan_params), loop g's env.step and
    plan read row g.  Returns (rollouts: per tick the list of M States, infos: per tick the last iteration's info, tick ms)."""
    import torch
    from dial_mpc_amd import _lib
    dc = mbdpi.args
    M = len(states)
    step_kw, plan_kw = {}, {}
    if user_params is not None:   # (padded device rows, converted once: each call binds them without a copy)
        rows = torch.as_tensor(_lib.plan_param_rows(user_params), device=mbdpi.device)
        if rows.shape[0] != M:
            raise ValueError(f"batched_loop: {rows.shape[0]} rows of task parameters for {M} closed loops")
        step_kw, plan_kw = dict(user_params=rows), dict(user_params=rows)
    rng = _generator(dc.seed, mbdpi.device)
    Y0 = torch.zeros((M, dc.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=mbdpi.device)
    rollouts, infos, tick_ms = [], [], []
    for t in range(n_steps):
        states = env.step_batch(states, Y0[:, 0], **step_kw)
        rollouts.append(states)
        t0 = time.time()
        Y0 = mbdpi.shift_batch(Y0)
        n_diffuse = dc.Ndiffuse_init if t == 0 else dc.Ndiffuse
        factors = mbdpi.sigma_control[None, :] * (dc.traj_diffuse_factor ** torch.arange(n_diffuse, device=mbdpi.device))[:, None]
        info = None
        for i in range(n_diffuse):
            eps = eps_fn(t, i) if eps_fn is not None else None
            rng, Y0, info = mbdpi.reverse_once_batch(states, rng, Y0, factors[i], eps=eps, want_bars=(i == n_diffuse - 1), **plan_kw)
        torch.cuda.synchronize()
        mbdpi.ctx.status()
        tick_ms.append((time.time() - t0) * 1e3)
        infos.append(info)
        if on_tick is not None:
            on_tick(t, states, tick_ms[-1])
    return rollouts, infos, tick_ms


def main_batched(dial_config, env, n_envs: int, env_params=None, model_kw=None):
    """``--n-envs M``: M closed loops from env.reset, each with its own plan noise, planned in one launch per annealing iteration.
    env_params: {name: [M values]} -- per-loop task parameters of a custom environment (``--env-param``).
    model_kw: MBDPI's models / model_of / model_per keywords (the YAML's plan_models block)."""
    print(f"Creating environment ({n_envs} closed loops, planned together)")
    rows = env.plan_params(**env_params) if env_params else None
    mbdpi = MBDPI(dial_config, env, n_plans=n_envs, **(model_kw or {}))
    states = [env.reset() for _ in range(n_envs)]

    def on_tick(t, sts, ms):
        if t % 20 == 0:
            print(f"step {t:4d}  rew {[round(float(s.reward), 3) for s in sts]}  tick {ms:.2f} ms")
    rollouts, infos, tick_ms = batched_loop(mbdpi, env, states, dial_config.n_steps, on_tick=on_tick, user_params=rows)
    for e in range(n_envs):
        print(f"env {e}: mean reward = {np.mean([float(r[e].reward) for r in rollouts]):.2e}")
    if len(tick_ms) > 1:
        print(f"batched tick (shift + Ndiffuse iterations, {n_envs} plans) p50 = {np.percentile(tick_ms[1:], 50):.3f} ms, "
              f"p95 = {np.percentile(tick_ms[1:], 95):.3f} ms")
    os.makedirs(dial_config.output_dir, exist_ok=True)
    timestamp = time.strftime("%Y%m%d-%H%M%S")
    per_env = [result_arrays([r[e] for r in rollouts], [{"xbar": inf["xbar"][e]} for inf in infos]) for e in range(n_envs)]
    np.save(os.path.join(dial_config.output_dir, f"{timestamp}_states"), np.stack([p[0] for p in per_env]))
    np.save(os.path.join(dial_config.output_dir, f"{timestamp}_predictions"), np.stack([p[1] for p in per_env]))


def result_arrays(rollout, infos):
    """The two artefacts of the reference's ``main`` (dial_core.py:305-323):
    ``states``      (n_steps, 1 + nq + nv + nu): [step index | qpos | qvel | ctrl] of every executed state;
    ``predictions`` (n_steps, Hsample+1, nbody-1, 3): the weighted-mean body positions ``xbar`` of the LAST annealing
    iteration of every tick -- upstream ``infos[i]["xbar"]`` comes out of ``lax.scan`` with a leading diffusion axis
    and ``[-1]`` selects that iteration; here ``infos[i]`` already is the last iteration's dict."""
    data, xdata = [], []
    for i, st in enumerate(rollout):
        ps = st.pipeline_state
        data.append(np.concatenate([[i], _np(ps.qpos), _np(ps.qvel), _np(ps.ctrl)]))
        xdata.append(_np(infos[i]["xbar"]))
    return np.array(data), np.array(xdata)


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


if __name__ == "__main__":
    main()
