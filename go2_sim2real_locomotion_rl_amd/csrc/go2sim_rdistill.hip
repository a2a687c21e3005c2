// go2sim_rdistill.hip -- teacher-student distillation with a recurrent student (include/go2sim_rdistill.h): the collection step in three launches and the
// behaviour-cloning update as truncated backpropagation through time over gradient windows.  gfx950 only.
//
// Every matrix kernel is shared: k_lstm_cell / k_lstm_bptt (go2sim_lstm_dev.h), k_mlp_forward / k_policy_sample (go2sim_mlp_dev.h), k_train_forward, k_bwd_*,
// k_reduce_partials, k_sumsq, k_adam (go2sim_train_dev.h, driven through go2sim_trainer_host.h) and the loss head with its float64 sums
// (go2sim_distill_dev.h).  What is new here are two row kernels and the schedule.  A window of P pairs over N envs is walked in env blocks of nb envs;
// one block is, on the caller's stream and without atomics,
//   k_rdistill_rows     the block's row list: workspace row p nb + j is rollout row t_p N + e0 + j, t_p from the window's segments
//   P x k_lstm_cell<true>   pair p steps on obs[t_p]; it enters with S (t_p = 0), the carried state (the window's first pair) or pair p - 1's h', c',
//                       masked by dones[t_p - 1]; gates and the entering state are kept
//   k_train_forward     the student on the P nb rows of h', then k_distill_head against the stored teacher actions, k_distill_finalize
//   launch_backward<.., true>   the student's layers; the first hands d loss / d h' back
//   P x k_lstm_bptt     from the last pair to the first; has_next = 0 at a segment's last step, cut = dones[t_p]
//   2 x (k_bwd_dw, k_bwd_db)    dW_ih and db_ih from x (rows through the list), dW_hh and db_hh from the entering h
//   k_reduce_partials   (one block) or k_distill_accumulate (several): the chunk slabs in chunk order in float64, kept across blocks, rounded once
//   k_rdistill_carry    the block's rows of the carried state [N][H]: pair P - 1's h', c' with dones[t_last] applied
// The optimizer is k_sumsq + k_adam<false> over student | memory_s: the memory's parameters sit where the PPO update keeps its critic's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <new>
#include <vector>

#define GO2SIM_MLP_ACT_KERNELS
#include "go2sim_mlp_dev.h"
#include "go2sim_lstm_dev.h"
#include "go2sim_train_dev.h"
#include "go2sim_distill_dev.h"
#define GO2SIM_HIPCHK_TAG "go2sim_rdistill"
#include "go2sim_trainer_host.h"
#include "../../include/go2sim_rdistill.h"

static_assert((int)GO2SIM_RDISTILL_GRADS == (int)GO2SIM_PPO_GRADS && (int)GO2SIM_RDISTILL_ADAM_M == (int)GO2SIM_PPO_ADAM_M && (int)GO2SIM_RDISTILL_ADAM_V == (int)GO2SIM_PPO_ADAM_V,
              "opt_vec serves this enum too");
static_assert((int)GO2SIM_RDISTILL_HUBER == (int)GO2SIM_DISTILL_HUBER && (int)GO2SIM_RDISTILL_N_STATS == (int)GO2SIM_DISTILL_N_STATS &&
              (int)GO2SIM_RDISTILL_ST_WINDOWS == (int)GO2SIM_DISTILL_ST_WINDOWS, "k_distill_head and k_distill_stats serve this header too");

namespace {

constexpr int MAXSEG = GO2SIM_RDISTILL_MAX_SEGS;

// a window's segments as the row kernel reads them: segment k holds the pairs [start[k], start[k + 1]) at steps t0[k], t0[k] + 1, ...
struct SegList { int n; int t0[MAXSEG]; int start[MAXSEG + 1]; };

// the rows of an env block in the rollout's arrays: idx[p nb + j] = t_p N + e0 + j
__global__ __launch_bounds__(WGT) void k_rdistill_rows(int32_t* __restrict__ idx, SegList s, int n, int nb, int N, int e0) {
  const int r = blockIdx.x * WGT + threadIdx.x;
  if (r >= n) return;
  const int p = r / nb, j = r - p * nb;
  int k = 0;
  while (k + 1 < s.n && s.start[k + 1] <= p) ++k;
  idx[r] = (s.t0[k] + (p - s.start[k])) * N + e0 + j;
}

// the carried state of nb envs: h', c' [nb][H] of the window's last pair, zero where `done` (u8 [nb]: dones[t_last]) is set
__global__ __launch_bounds__(WGT) void k_rdistill_carry(const float* __restrict__ hsrc, const float* __restrict__ csrc, const uint8_t* __restrict__ done,
                                                        float* __restrict__ hdst, float* __restrict__ cdst, int nb, int H) {
  const size_t i = (size_t)blockIdx.x * WGT + threadIdx.x;
  if (i >= (size_t)nb * H) return;
  const bool keep = !done[i / H];
  hdst[i] = keep ? hsrc[i] : 0.0f;
  cdst[i] = keep ? csrc[i] : 0.0f;
}

}  // namespace

struct go2sim_rdistill {
  go2sim_lstm* mem = nullptr;
  go2sim_mlp* student = nullptr;
  go2sim_rdistill_cfg_t cfg{};
  int A = 0, Apad = 0, sub = 0;
  size_t R = 0;               // workspace rows
  size_t nS = 0, nM = 0, nP = 0, n_flat = 0;   // padded student, memory, both; flat size
  OptState opt;               // over nP floats; its tail: acc[nP] | head partials
  float* wbuf = nullptr;      // mu | the student's row workspaces | chunk slabs | the memory's row workspaces, for R rows
  int32_t* ibuf = nullptr;    // idx [R] (rows of the block in the rollout's arrays) | idx_id [R] (0 .. R - 1)
  float *mu = nullptr, *partial = nullptr;
  NetWs nw{};
  float *gates = nullptr, *dz = nullptr, *hprev = nullptr, *cprev = nullptr, *hout = nullptr, *cout = nullptr, *dh = nullptr, *dc = nullptr;
  int32_t *idx = nullptr, *idx_id = nullptr;
  double *acc = nullptr, *head_part = nullptr;
  long long pairs = 0, windows = 0;
  std::vector<Seg> segs;      // base 0 student, 1 memory_s
};

namespace {

void vec_bases(go2sim_rdistill* h, int which, float** base) {
  if (which == GO2SIM_RDISTILL_PARAMS) { base[0] = h->student->dparams; base[1] = h->mem->dparams; return; }
  float* v = opt_vec(h->opt, which);
  base[0] = v; base[1] = v ? v + h->nS : nullptr;
}

bool roll_ok(const go2sim_rdistill_roll_t* r) {
  return r && r->obs && r->teacher_actions && r->dones && r->h0 && r->c0 && r->h && r->c && r->h != r->h0 && r->c != r->c0 && r->n_steps >= 1 && r->n_envs >= 1 &&
         (long long)r->n_steps * r->n_envs <= 0x7fffffffLL / MAXW;
}

// the segments of one window, checked: -> pairs, 0 when the list is not one
int seg_list(const go2sim_rdistill_seg_t* segs, int n_segs, int T, SegList& s) {
  if (!segs || n_segs < 1 || n_segs > MAXSEG) return 0;
  int P = 0;
  for (int k = 0; k < n_segs; ++k) {
    if (segs[k].n_steps < 1 || segs[k].t0 < 0 || segs[k].t0 > T - segs[k].n_steps || (k > 0 && segs[k].t0 != 0)) return 0;
    s.t0[k] = segs[k].t0; s.start[k] = P;
    if (segs[k].n_steps > 0x7fffffff - P) return 0;
    P += segs[k].n_steps;
  }
  s.n = n_segs; s.start[n_segs] = P;
  return P;
}

// One window (see the head of this file).  `backward`: the gradient as well; otherwise forward, head and state alone.
int launch_window(go2sim_rdistill* h, const go2sim_rdistill_roll_t* roll, const SegList& s, bool backward, hipStream_t st) {
  const go2sim_mlp* M = h->student;
  const go2sim_lstm* m = h->mem;
  const int T = roll->n_steps, N = roll->n_envs, P = s.start[s.n];
  const size_t H = m->H, Hp = m->dev.Hpad, I = m->I;
  const int nb_max = N < h->sub ? N : h->sub, n_blocks = (N + nb_max - 1) / nb_max;
  const double w = 1.0 / ((double)N * (double)h->A);
  const int groups = ((int)Hp / 16 + NWAVE - 1) / NWAVE;
  const size_t slab = h->nP;
  std::vector<int> step(P), last(P);                       // pair p's step, and whether it is its segment's last
  for (int k = 0; k < s.n; ++k)
    for (int p = s.start[k]; p < s.start[k + 1]; ++p) { step[p] = s.t0[k] + (p - s.start[k]); last[p] = p == s.start[k + 1] - 1; }
  (void)T;
  for (int blk = 0; blk < n_blocks; ++blk) {
    const int e0 = blk * nb_max, nb = N - e0 < nb_max ? N - e0 : nb_max, n = P * nb;
    hipLaunchKernelGGL(k_rdistill_rows, dim3((n + WGT - 1) / WGT), dim3(WGT), 0, st, h->idx, s, n, nb, N, e0);
    for (int p = 0; p < P; ++p) {
      const int t = step[p];
      const size_t o = (size_t)p * nb;
      CellNet c[2] = {};
      CellNet& C = c[0];
      C.M = m->dev; C.x = roll->obs + ((size_t)t * N + e0) * I; C.ldx = (int)I;
      if (t == 0) { C.hin = roll->h0 + (size_t)e0 * H; C.cin = roll->c0 + (size_t)e0 * H; }
      else if (p == 0) { C.hin = roll->h + (size_t)e0 * H; C.cin = roll->c + (size_t)e0 * H; }
      else { C.hin = h->hout + (o - nb) * H; C.cin = h->cout + (o - nb) * H; }
      C.hout = h->hout + o * H; C.cout = h->cout + o * H;
      C.gates = h->gates + o * 4 * Hp; C.hprev = h->hprev + o * H; C.cprev = h->cprev + o * H;
      C.active = 1;
      hipLaunchKernelGGL(k_lstm_cell<true>, dim3((nb + TM - 1) / TM, groups, 1), dim3(64 * NWAVE), 0, st, c[0], c[1],
                         t == 0 ? (const uint8_t*)nullptr : roll->dones + (size_t)(t - 1) * N + e0, nb);
    }
    hipLaunchKernelGGL(k_train_forward<false>, dim3((n + TM - 1) / TM, 1), dim3(64 * NWAVE), 0, st, M->dev, h->hout, h->mu, h->nw.a, M->dev, h->hout, h->mu, h->nw.a, h->idx_id,
                       n, n, MirTab{nullptr, nullptr}, MirTab{nullptr, nullptr});
    DistillHeadArgs ha{};
    ha.mu = h->mu; ha.teacher = roll->teacher_actions; ha.idx = h->idx; ha.dz = h->nw.dz[(M->n_layers - 1) & 1]; ha.part = h->head_part;
    ha.n = n; ha.A = h->A; ha.Apad = h->Apad; ha.huber = h->cfg.loss_type == GO2SIM_RDISTILL_HUBER; ha.w = w;
    const int n_wg = (n + WGT - 1) / WGT;
    hipLaunchKernelGGL(k_distill_head, dim3(n_wg), dim3(WGT), 0, st, ha);
    hipLaunchKernelGGL(k_distill_finalize, dim3(1), dim3(1), 0, st, h->head_part, n_wg, w, h->opt.scal);
    if (backward) {
      BwdLayer L[MAXL][2] = {};                              // the second network's slot of the shared kernels stays empty
      for (int lb = 0; lb < M->n_layers; ++lb) {
        BwdLayer& Q = L[lb][0];
        Q = bwd_layer(M, h->nw, lb, h->hout, 0, MirTab{nullptr, nullptr}, 0);
        if (M->n_layers - 1 - lb == 0) { Q.dzprev = h->dh; Q.lin = 1; }   // the first layer reads the memory's h' [n][H] and hands d loss / d h' back
      }
      launch_backward<false, true>(L, M->n_layers, BwdRun{1, h->idx_id, n, n, h->partial, slab, st});
      for (int p = P - 1; p >= 0; --p) {
        const size_t o = (size_t)p * nb;
        BpttNet b[2] = {};
        BpttNet& B = b[0];
        B.M = m->dev; B.dz_next = h->dz + (o + nb) * 4 * Hp; B.dh_mlp = h->dh + o * Hp; B.gates = h->gates + o * 4 * Hp;
        B.cprev = h->cprev + o * H; B.cout = h->cout + o * H; B.dc = h->dc; B.dz = h->dz + o * 4 * Hp; B.active = 1;
        hipLaunchKernelGGL(k_lstm_bptt, dim3((nb + TM - 1) / TM, groups, 1), dim3(64 * NWAVE), 0, st, b[0], b[1], roll->dones + (size_t)step[p] * N + e0, last[p] ? 0 : 1, nb);
      }
      // the memory's weight gradients over the block's n rows: dW_ih = dz^T x (rows through the list), dW_hh = dz^T h_prev, db_ih = db_hh = column sums of dz
      const size_t o_hh = 4 * Hp * (size_t)m->dev.Ipad, o_bi = o_hh + 4 * Hp * Hp;
      for (int part = 0; part < 2; ++part) {
        BwdLayer Q{}, none{};
        Q.active = 1; Q.dz = h->dz; Q.N = 4 * (int)Hp;
        if (part == 0) { Q.aprev = roll->obs; Q.K = m->dev.Ipad; Q.lda = m->I; Q.kmax = m->I; Q.gather = 1; Q.W = m->dev.Wih; Q.w_off = h->nS; Q.b_off = h->nS + o_bi; }
        else { Q.aprev = h->hprev; Q.K = (int)Hp; Q.lda = m->H; Q.kmax = m->H; Q.gather = 0; Q.W = m->dev.Whh; Q.w_off = h->nS + o_hh; Q.b_off = h->nS + o_bi + 4 * Hp; }
        launch_dw_db<false>(Q, none, BwdRun{1, h->idx, n, n, h->partial, slab, st});
      }
      const int n_chunks = (n + RCH - 1) / RCH;
      const dim3 grid((unsigned)((slab + WGT - 1) / WGT));
      if (n_blocks == 1) hipLaunchKernelGGL(k_reduce_partials, grid, dim3(WGT), 0, st, h->partial, n_chunks, slab, h->opt.grads);
      else hipLaunchKernelGGL(k_distill_accumulate, grid, dim3(WGT), 0, st, h->partial, n_chunks, slab, h->acc, blk == 0 ? 1 : 0, blk == n_blocks - 1 ? 1 : 0, h->opt.grads);
    }
    const size_t o = (size_t)(P - 1) * nb;
    hipLaunchKernelGGL(k_rdistill_carry, dim3((unsigned)(((size_t)nb * H + WGT - 1) / WGT)), dim3(WGT), 0, st, h->hout + o * H, h->cout + o * H,
                       roll->dones + (size_t)step[P - 1] * N + e0, roll->h + (size_t)e0 * H, roll->c + (size_t)e0 * H, nb, (int)H);
  }
  HIPCHK(hipGetLastError());
  h->pairs += P;
  return GO2SIM_E_OK;
}

int window_call(go2sim_rdistill_t* h, const go2sim_rdistill_roll_t* roll, const go2sim_rdistill_seg_t* segs, int n_segs, bool backward, void* stream) {
  if (!h || !roll_ok(roll)) return GO2SIM_E_BADARG;
  SegList s{};
  const int P = seg_list(segs, n_segs, roll->n_steps, s);
  const int nb = roll->n_envs < h->sub ? roll->n_envs : h->sub;
  if (P < 1 || (long long)P * nb > (long long)h->R) return GO2SIM_E_BADARG;
  return launch_window(h, roll, s, backward, (hipStream_t)stream);
}

int pack_all(go2sim_rdistill* h, int which, int to_padded, float* flat, hipStream_t st) {
  if (!h || !flat || which < GO2SIM_RDISTILL_PARAMS || which > GO2SIM_RDISTILL_ADAM_V) return GO2SIM_E_BADARG;
  float* base[2];
  vec_bases(h, which, base);
  return pack_segs(h->segs, base, to_padded, flat, st);
}

}  // namespace

extern "C" {

int go2sim_rdistill_act(go2sim_lstm_t* mem_s, go2sim_mlp_t* student, go2sim_lstm_t* mem_t, go2sim_mlp_t* teacher, const float* obs, const float* teacher_obs,
                        const float* std_dev, const uint8_t* reset, const float* h_in_s, const float* c_in_s, float* h_out_s, float* c_out_s, const float* h_in_t,
                        const float* c_in_t, float* h_out_t, float* c_out_t, int n_rows, uint64_t seed, uint32_t step, int deterministic, float* actions, float* mean,
                        float* teacher_actions, void* stream) {
  if (!mem_s || !student || !teacher || !obs || !teacher_obs || !std_dev || !h_in_s || !c_in_s || !h_out_s || !c_out_s || h_out_s == h_in_s || !actions || !mean ||
      !teacher_actions || n_rows < 0)
    return GO2SIM_E_BADARG;
  if (mem_t && (!h_in_t || !c_in_t || !h_out_t || !c_out_t || h_out_t == h_in_t)) return GO2SIM_E_BADARG;
  const int A = student->dims[student->n_layers];
  if (teacher->dims[teacher->n_layers] != A || teacher->device != student->device || mem_s->device != student->device || mem_s->H != student->dims[0]) return GO2SIM_E_BADARG;
  if (mem_t && (mem_t->device != student->device || mem_t->H != teacher->dims[0])) return GO2SIM_E_BADARG;
  if (n_rows == 0) return GO2SIM_E_OK;
  hipStream_t st = (hipStream_t)stream;
  CellNet c[2] = {};
  c[0].M = mem_s->dev; c[0].x = obs; c[0].ldx = mem_s->I; c[0].hin = h_in_s; c[0].cin = c_in_s; c[0].hout = h_out_s; c[0].cout = c_out_s; c[0].active = 1;
  int groups = (mem_s->dev.Hpad / 16 + NWAVE - 1) / NWAVE;
  if (mem_t) {
    c[1].M = mem_t->dev; c[1].x = teacher_obs; c[1].ldx = mem_t->I; c[1].hin = h_in_t; c[1].cin = c_in_t; c[1].hout = h_out_t; c[1].cout = c_out_t; c[1].active = 1;
    const int g = (mem_t->dev.Hpad / 16 + NWAVE - 1) / NWAVE;
    if (g > groups) groups = g;
  }
  hipLaunchKernelGGL(k_lstm_cell<false>, dim3((n_rows + TM - 1) / TM, groups, mem_t ? 2 : 1), dim3(64 * NWAVE), 0, st, c[0], c[1], reset, n_rows);
  hipLaunchKernelGGL(k_mlp_forward, dim3((n_rows + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, student->dev, (const float*)h_out_s, mean, teacher->dev,
                     mem_t ? (const float*)h_out_t : teacher_obs, teacher_actions, n_rows);
  hipLaunchKernelGGL(k_policy_sample, dim3((n_rows + 63) / 64), dim3(64), 0, st, mean, std_dev, n_rows, A, seed, step, deterministic, actions, (float*)nullptr);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_rdistill_create(go2sim_lstm_t* mem_s, go2sim_mlp_t* student, int n_actions, const go2sim_rdistill_cfg_t* cfg, int max_window_rows, go2sim_rdistill_t** out) {
  if (!mem_s || !student || !cfg || !out || max_window_rows < 1 || n_actions < 1 || student->dims[student->n_layers] != n_actions) return GO2SIM_E_BADARG;
  if (mem_s->H != student->dims[0] || mem_s->device != student->device || (long long)max_window_rows > 0x7fffffffLL / 4 / MAXW) return GO2SIM_E_BADARG;
  if (!(cfg->learning_rate > 0.0) || (cfg->loss_type != GO2SIM_RDISTILL_MSE && cfg->loss_type != GO2SIM_RDISTILL_HUBER)) return GO2SIM_E_BADARG;
  if (cfg->sub_envs < 0 || std::isnan(cfg->max_grad_norm)) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(student->device));
  go2sim_rdistill* h = new (std::nothrow) go2sim_rdistill();
  if (!h) return GO2SIM_E_NOMEM;
  const go2sim_mlp* M = student;
  h->mem = mem_s; h->student = student; h->cfg = *cfg; h->A = n_actions; h->Apad = round16(n_actions);
  h->sub = cfg->sub_envs ? cfg->sub_envs : GO2SIM_RDISTILL_SUB_ENVS;
  h->R = (size_t)max_window_rows;
  h->nS = M->padded; h->nM = mem_s->padded; h->nP = h->nS + h->nM;
  mlp_segs(h->segs, 0, M, h->n_flat);
  lstm_segs(h->segs, 1, mem_s, h->n_flat);
  const size_t R = h->R, H = mem_s->H, Hp = mem_s->dev.Hpad;
  const int chunks = (int)((R + RCH - 1) / RCH), head_wg = (int)((R + WGT - 1) / WGT);
  const size_t need = al16(R * h->A) + net_ws_floats(M, R) + (size_t)chunks * h->nP + 2 * al16(R * 4 * Hp) + 4 * al16(R * H) + 2 * al16(R * Hp);
  if (!opt_alloc(h->opt, h->nP, h->nP + (size_t)head_wg) || hipMalloc((void**)&h->wbuf, need * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&h->ibuf, 2 * R * sizeof(int32_t)) != hipSuccess) {
    go2sim_rdistill_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  if (!opt_zero(h->opt, cfg->learning_rate, h->wbuf, need)) {
    fprintf(stderr, "go2sim_rdistill: initialising the trainer failed: %s\n", hipGetErrorString(hipGetLastError()));
    go2sim_rdistill_destroy(h);
    return GO2SIM_E_HIP;
  }
  h->acc = h->opt.tail; h->head_part = h->acc + h->nP;
  h->mu = h->wbuf;
  float* p = net_ws_carve(M, R, h->mu + al16(R * h->A), h->nw);
  h->partial = p; p += (size_t)chunks * h->nP;
  h->gates = p; p += al16(R * 4 * Hp); h->dz = p; p += al16(R * 4 * Hp);
  h->hprev = p; p += al16(R * H); h->cprev = p; p += al16(R * H); h->hout = p; p += al16(R * H); h->cout = p; p += al16(R * H);
  h->dh = p; p += al16(R * Hp); h->dc = p;
  h->idx = h->ibuf; h->idx_id = h->ibuf + R;
  hipLaunchKernelGGL(k_iota, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, 0, h->idx_id, (int)R);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    go2sim_rdistill_destroy(h);
    return GO2SIM_E_HIP;
  }
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_rdistill_destroy(go2sim_rdistill_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  opt_free(h->opt);
  if (h->wbuf) (void)hipFree(h->wbuf);
  if (h->ibuf) (void)hipFree(h->ibuf);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_rdistill_window_grad(go2sim_rdistill_t* h, const go2sim_rdistill_roll_t* roll, const go2sim_rdistill_seg_t* segs, int n_segs, void* stream) {
  return window_call(h, roll, segs, n_segs, true, stream);
}

int go2sim_rdistill_loss_only(go2sim_rdistill_t* h, const go2sim_rdistill_roll_t* roll, const go2sim_rdistill_seg_t* segs, int n_segs, void* stream) {
  return window_call(h, roll, segs, n_segs, false, stream);
}

int go2sim_rdistill_apply(go2sim_rdistill_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  AdamArgs a{};
  a.p_actor = h->student->dparams; a.nA = h->nS;
  a.p_critic = h->mem->dparams; a.nC = h->nM;               // the memory's block follows the student's, as the critic's follows the actor's
  a.max_norm = h->cfg.max_grad_norm > 0.0 ? h->cfg.max_grad_norm : std::numeric_limits<double>::infinity();   // no clip: the coefficient is min(1, inf) = 1, exact
  a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.eps;
  const int rc = opt_apply<false>(h->opt, a, (hipStream_t)stream);
  if (rc == GO2SIM_E_OK) h->windows += 1;
  return rc;
}

int go2sim_rdistill_update(go2sim_rdistill_t* h, const go2sim_rdistill_roll_t* roll, int E, int G, void* stream) {
  if (!h || !roll_ok(roll) || E < 1 || G < 1) return GO2SIM_E_BADARG;
  const int T = roll->n_steps, nb = roll->n_envs < h->sub ? roll->n_envs : h->sub;
  const long long pairs = (long long)E * T;
  if ((long long)G * nb > (long long)h->R || pairs > 0x7fffffffLL) return GO2SIM_E_BADARG;
  // the schedule: the pairs in order, a window closes at every multiple of G; every window's segment list is checked before the first launch
  std::vector<std::vector<go2sim_rdistill_seg_t>> wins(1);
  long long cnt = 0;
  for (int e = 0; e < E; ++e)
    for (int t = 0; t < T; ++t) {
      std::vector<go2sim_rdistill_seg_t>& cur = wins.back();
      if (cur.empty() || t == 0) cur.push_back(go2sim_rdistill_seg_t{t, 1});
      else cur.back().n_steps += 1;
      if (++cnt % G == 0) wins.emplace_back();
    }
  for (const auto& wd : wins)
    if (wd.size() > (size_t)MAXSEG) return GO2SIM_E_BADARG;
  int rc = go2sim_rdistill_reset_stats(h, stream);
  for (size_t i = 0; i < wins.size() && rc == GO2SIM_E_OK; ++i) {
    if (wins[i].empty()) continue;                          // the open window after the last close holds no pair
    const bool tail = i + 1 == wins.size();
    rc = window_call(h, roll, wins[i].data(), (int)wins[i].size(), !tail, stream);
    if (rc == GO2SIM_E_OK && !tail) rc = go2sim_rdistill_apply(h, stream);
  }
  return rc;
}

int go2sim_rdistill_n_params(go2sim_rdistill_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->n_flat;
  return GO2SIM_E_OK;
}
int go2sim_rdistill_export(go2sim_rdistill_t* h, int which, float* flat_dev, void* stream) { return pack_all(h, which, 0, flat_dev, (hipStream_t)stream); }
int go2sim_rdistill_import(go2sim_rdistill_t* h, int which, const float* flat_dev, void* stream) {
  return pack_all(h, which, 1, const_cast<float*>(flat_dev), (hipStream_t)stream);
}
int go2sim_rdistill_n_padded(go2sim_rdistill_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->nP;
  return GO2SIM_E_OK;
}
int go2sim_rdistill_export_padded(go2sim_rdistill_t* h, int which, float* padded_dev, void* stream) {
  if (!h || !padded_dev || which < GO2SIM_RDISTILL_PARAMS || which > GO2SIM_RDISTILL_ADAM_V) return GO2SIM_E_BADARG;
  float* base[2];
  vec_bases(h, which, base);
  HIPCHK(hipMemcpyAsync(padded_dev, base[0], h->nS * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIPCHK(hipMemcpyAsync(padded_dev + h->nS, base[1], h->nM * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GO2SIM_E_OK;
}

int go2sim_rdistill_set_step(go2sim_rdistill_t* h, long long step, double learning_rate, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  return opt_set_step(h->opt, step, learning_rate, (hipStream_t)stream);
}
int go2sim_rdistill_reset_stats(go2sim_rdistill_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_reset, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal);
  HIPCHK(hipGetLastError());
  h->pairs = 0; h->windows = 0;
  return GO2SIM_E_OK;
}
int go2sim_rdistill_stats(go2sim_rdistill_t* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal, (double)h->opt.step, (double)h->pairs, (double)h->windows, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"
