/* go2sim_cterms.h -- C ABI and law of the two CONTACT TERMS: reward terms of the reference that read the links' net contact forces and that the
 * step kernels do not have:
 *   body_contact   examples/locomotion/go2_env_stair_lidar_2.py (_init_body_contact_tracking :1098, _reward_body_contact :1865): the number of
 *                  listed links (the script: the two front thighs) whose contact force exceeds a threshold -- the term that keeps the robot from
 *                  crawling up the treads on its thighs;
 *   stumble        examples/locomotion/go2_env_terrain.py (_reward_stumble :1380): the contact force above a threshold, summed over every robot link
 *                  that is not a foot -- the rough-terrain counterpart.
 * Both read the same 13 x 3 floats per env, so one launch serves both.  They live here and not in the step kernels because the core's reward ids are
 * pinned (GO2SIM_R_COUNT); the form is the stairwell env's alive term's (include/go2sim_wells.h): a small launch after the step's own that adds to
 * `rew`, keeps its own episode sums and hands them over on reset.
 *
 * Conventions follow go2sim_wells.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given
 * stream, no call below synchronises with the host unless it says so.  Product library only: there is no CPU twin, the checker is the numpy float64
 * restatement tests/cterms_ref.py, itself pinned to the reference's own methods (tests/golden/ref_cterms.npz, tools/make_ref_cterms_fixtures.py).
 *
 * ---- The law ----
 * Link numbering is the model's: link 0 is the ground, links 1 .. n_links - 1 are the robot (Go2: n_links = 14; the feet are the four calf links).
 * Bit l of a mask selects link l.  F_l = (Fx, Fy, Fz) is the float32 net contact force of link l (GO2SIM_F_CONTACT_FORCE: what the last substep's
 * solve committed; the reset path does not touch it, so after go2sim_env_step it holds the forces the reference's reward reads before its reset_idx,
 * for the envs reset in that step too).  Everything is float32, IEEE operations in the written order, no contraction:
 *   n_l = dm_sqrt((Fx Fx + Fy Fy) + Fz Fz)                                    three rounded products, two rounded sums, the correctly rounded root
 *
 *   body_contact:   count = sum over l in body_mask of (n_l > f32(body_contact_threshold) ? 1 : 0)       a NaN norm compares false
 *                   term_b = f32(count) * inc_b,          inc_b = f32(body_contact_scale * dt)           the product in float64, rounded once
 *   stumble:        pen = sum over l in stumble_mask, ascending l, of max(n_l - f32(stumble_threshold), 0)
 *                   (d = n_l - thr;  d < 0 ? 0 : d -- a NaN stays, as torch's clamp(min=0) keeps it; the sum starts at 0 and adds link by link)
 *                   term_s = pen * inc_s,                 inc_s = f32(stumble_scale * dt)
 * (the reference multiplies a float32 tensor by the python float scale * dt.)  With rew != NULL, for every env b, first body_contact, then stumble,
 * each only if its scale is not zero:
 *   rew[b] = rew[b] + term;   sum_t[b] = sum_t[b] + term;   steps_t[b] += 1
 * and for an env whose reset flag is set, after that, per applied term -- the alive term's hand-over:
 *   ep_t[b] = sum_t[b] / (f32(max(steps_t[b], 1)) * f32(dt));   sum_t[b] = 0;   steps_t[b] = 0
 * extras["episode"]["rew_body_contact"] / ["rew_stumble"] are the means of ep_t over the envs of the last reset, as the core's terms are reported.
 * count_out[b] = f32(count) is written on every call (with either scale, with rew NULL): the last step's count, for evaluation code that reports a
 * crawl rate.  In a stairwell env the wells launch runs first: alive, then body_contact, then stumble.
 *
 * CONSEQUENCE: the terms are added after the core's sum, whatever their place in reward_scales, while the reference adds the terms in dictionary
 * order.  body_contact is last in the script's dictionary, so there the float32 total is the reference's to the bit; elsewhere in a dictionary it can
 * differ in the last place.
 *
 * Safety and determinism.  The launch reads, per env, the three components of every link in either mask at
 * cf[comp * comp_stride + link * link_stride + b * env_stride] and nothing else of cf: the caller's strides and n_links bound the reads.  No LDS, no
 * atomics, no data-dependent trip counts: equal calls give equal bits on any stream.
 *
 * Launch (csrc/go2sim_cterms.hip): k_cterms_step, one per call: one lane per env, 256-lane workgroups.  The link loop runs over the
 * GO2SIM_CTERMS_LINKS_MAX bit positions, unrolled, and skips the links in neither mask (a wave-uniform test of a handle constant).  In the pool's
 * layout (comp_stride = n_envs, link_stride = 3 n_envs, env_stride = 1) every load is coalesced over the wavefront.
 */
#ifndef GO2SIM_CTERMS_H
#define GO2SIM_CTERMS_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_CTERMS_LINKS_MAX 32 /* links a mask can name */
#define GO2SIM_CTERMS_BODY 0       /* index of body_contact in the per-term arrays */
#define GO2SIM_CTERMS_STUMBLE 1    /* index of stumble */
#define GO2SIM_CTERMS_N 2

typedef struct go2sim_cterms go2sim_cterms_t;

typedef struct {
  double dt;                                        /* the env step */
  double body_contact_scale, stumble_scale;         /* reward_scales[...]; 0: the term is not applied */
  double body_contact_threshold, stumble_threshold; /* newtons */
  int n_envs, n_links;
  uint32_t body_mask, stumble_mask; /* bit l: link l */
} go2sim_cterms_cfg_t;

/* GO2SIM_E_BADARG: n_envs < 1, n_links outside [1, 32], a mask bit at or above n_links, dt <= 0 or a NaN constant.  Sums, step counts and records
 * start at 0.  Waits for the device. */
int go2sim_cterms_create(int device, const go2sim_cterms_cfg_t* cfg, go2sim_cterms_t** out);
int go2sim_cterms_destroy(go2sim_cterms_t* h);

/* One step of all n == n_envs envs: one launch.  cf: float32 device memory, component c of link l of env b at
 * cf[c * comp_stride + l * link_stride + b * env_stride] (elements): the pool's SoA field is (n, 3 n, 1), a row-major [n][n_links][3] tensor
 * (1, 3, 3 n_links).  reset: uint8 [n] or NULL (no env was reset).  rew: float32 [n], updated in place, or NULL: nothing is added, sums, counts and
 * records stay.  count_out: float32 [n] or NULL.
 * GO2SIM_E_BADARG -- nothing is launched -- for a NULL handle or cf, n != n_envs and negative strides. */
int go2sim_cterms_step(go2sim_cterms_t* h, int n, const float* cf, long long comp_stride, long long link_stride, long long env_stride,
                       const uint8_t* reset, float* rew, float* count_out, void* stream);

/* The episode hand-over of the law above without a step, of both terms, for the n_sel envs of envs_idx (int32, device memory; entries outside
 * [0, n_envs) are passed over) or for all envs when envs_idx is NULL (Go2Env.reset / reset_idx).  One launch. */
int go2sim_cterms_clear(go2sim_cterms_t* h, const int* envs_idx, int n_sel, void* stream);

/* sum float32 [2][n_envs], steps int32 [2][n_envs], ep float32 [2][n_envs] (term GO2SIM_CTERMS_BODY, then GO2SIM_CTERMS_STUMBLE), host memory;
 * bit-exact both ways.  Both wait for the stream. */
int go2sim_cterms_get_state(go2sim_cterms_t* h, float* sum, int32_t* steps, float* ep, void* stream);
int go2sim_cterms_set_state(go2sim_cterms_t* h, const float* sum, const int32_t* steps, const float* ep, void* stream);

/* device addresses of the two ep arrays, float32 [n_envs] each, for the host to reduce in place; the two inc values as the kernel multiplies them */
int go2sim_cterms_ep(go2sim_cterms_t* h, const float** body_ep_dev, const float** stumble_ep_dev, float* inc_body, float* inc_stumble);

#ifdef __cplusplus
}
#endif
#endif
