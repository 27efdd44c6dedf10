// unread_emu.cpp -- host wave emulator of the Go2 rollout on a Wave (every solver pass, every phase of every step) and on a WaveD
// (wave.h: deferred step rewards, the Newton loop's exit at the iteration cap, the cut last step of a lean rollout)
// (TEST INFRASTRUCTURE ONLY).
//
// defer_emu.cpp's harness (same LDS image, same race detector) with two additions: any of qss / qdss / xss may be null -- a rollout
// that stores neither q nor qd is a lean one, whose last step WaveD cuts -- and the solver's exit hook (solver_reg.h) counts the
// solves that end by tolerance and the solves that end with niter at the iteration cap, so that a test can tell that its inputs
// exercise both.  (With the race detector on, a solve is still one call: the detector re-runs items() phases, not the solver.)
#define DIAL_EMU 1
namespace {
int g_exit_tol = 0, g_exit_cap = 0;
}
#define DIAL_SOLVER_EXIT_HOOK(at_cap) ((at_cap) ? ++g_exit_cap : ++g_exit_tol)
#include "../../dial_mpc_amd/csrc/rollout_driver.h"

#include <type_traits>
#include <vector>

namespace {

template <bool DEFER>
int run(const dial_model* m, const dial_task* t, const dial_derived* dv, const dial_cfg* cfg, const dial::RolloutIO& io, int B, int check_races) {
  using D = DimsGo2;
  static CModel<D> cm;
  fill_cmodel(&cm, m, t, dv);
  Ws s0;
  const int ws_words = ws_carve(s0, (float*)0, m->nq, m->nv, m->nu, m->nbody, m->njnt, m->ngeom, m->nsite, m->ncon, m->nefc, DIAL_MAX_NODE,
                                dial::kNeedL<D>, D::square, 0, 0, D::NVP, DIAL_MAX_T);
  const int stash_words = DEFER ? io.T * DIAL_REWARD_STASH_W : 0;
  int races = 0;
  for (int n = 0; n < B; n++) {
    std::vector<float> lds(ws_words + stash_words, 0.f);
    Ws s;
    ws_carve(s, lds.data(), cm.nq, cm.nv, cm.nu, cm.nbody, cm.njnt, cm.ngeom, cm.nsite, cm.ncon, cm.nefc, DIAL_MAX_NODE, dial::kNeedL<D>,
             D::square, 0, 0, D::NVP, DIAL_MAX_T);
    std::conditional_t<DEFER, WaveD, Wave> w;
    static_assert(!DEFER || (decltype(w)::solver_cap_exit && decltype(w)::lean_tail_cut), "the twin of the kernel as shipped");
    w.lds = lds.data();
    w.lds_words = ws_words + stash_words;
    w.check_races = check_races != 0;
    if constexpr (DEFER) {
      w.stash = lds.data() + ws_words;
      w.zbase = w.stash + 16 * io.T;
    }
    dial::rollout_sample<false>(w, &cm, t, cfg, s, io, n);
    races += w.races;
  }
  return races;
}

}  // namespace

// exits[0] / exits[1]: solves of this call that ended by tolerance / with niter at the iteration cap
extern "C" int unread_emu_rollout(const dial_model* m, const dial_task* t, const dial_cfg* cfg, const float* state, const float* eps,
                                  const float* Ybar, const float* noise_scale, int ns, int n_noise, int B, int T, int Hn1, float* Y0s,
                                  float* rewss, float* rews, float* qss, float* qdss, float* xss, int check_races, int defer, int* exits) {
  dial_derived dv;
  if (int rc = dial_build_derived(m, &dv)) return -1000 - rc;
  if (!dims_match<DimsGo2>(m) || t->kind != DIAL_TASK_GO2_WALK) return -1;
  // (what dial_create asks of the task before it launches the deferring kernel: the position stage stores the trunk's and the calves' words)
  if (t->torso_x != 0 || t->upright_x != 0 || t->nfeet != 4) return -2;
  for (int f = 0; f < 4; f++) if (t->feet_site[f] < 1 || t->feet_site[f] > 4) return -2;
  dial::RolloutIO io{state, nullptr, eps, Ybar, noise_scale, ns, n_noise, T, Hn1, Y0s, rewss, rews, qss, qdss, xss, nullptr, 0, 0u, 0u, 0u, 0};
  g_exit_tol = g_exit_cap = 0;
  const int rc = defer ? run<true>(m, t, &dv, cfg, io, B, check_races) : run<false>(m, t, &dv, cfg, io, B, check_races);
  exits[0] = g_exit_tol;
  exits[1] = g_exit_cap;
  return rc;
}
