/* go2sim_activation.h -- C ABI of the hidden-layer activation of one MLP (include/go2sim_policy.h): the seven names rsl_rl's
 * `resolve_nn_activation` (rsl-rl-lib==2.2.4) maps to a torch module that is a function of one value.  rsl_rl is a third-party package that is not
 * part of the reference tree; the torch modules are the contract.  Product library only: there is no CPU twin, the checker is numpy float64
 * (tests/act_ref.py).
 *
 * The activation is a property of one go2sim_mlp_t: the two networks of one launch (actor / critic, student / teacher) may differ.  It is applied
 * after every layer but the last; a first layer behind a memory (include/go2sim_rnn.h) reads the memory's h, which is no activation's output.  A new
 * MLP is GO2SIM_ACT_ELU, and with it every entry point computes the bits it computed before this header existed.
 *
 *   name      module             forward a = f(v)                                       derivative, from the stored post-activation a
 *   elu       nn.ELU()           v > 0 ? v : exp(v) - 1                                 a > 0 ? 1 : a + 1
 *   selu      nn.SELU()          v > 0 ? L v : L A (exp(v) - 1)                         a > 0 ? L : a + L A
 *   relu      nn.ReLU()          v < 0 ? 0 : v                                          a > 0 ? 1 : 0
 *   lrelu     nn.LeakyReLU()     v > 0 ? v : 0.01 v                                     a > 0 ? 1 : 0.01
 *   tanh      nn.Tanh()          sign(v) (1 - e) / (1 + e),  e = exp(-2 |v|)            1 - a a
 *   sigmoid   nn.Sigmoid()       e = exp(-|v|):  v >= 0 ? 1 / (1 + e) : e / (1 + e)     a (1 - a)
 *   identity  nn.Identity()      v                                                      1
 * L = 1.0507009873554805, A = 1.6732632423543772 (torch's SELU constants; L, L A and 0.01 are rounded to float32 once).  `crelu`, which rsl_rl also
 * lists, doubles the layer's width and is not a function of one value: the Python classes refuse it by name.
 *
 * Every derivative is a function of the post-activation alone, so the update keeps what it kept for ELU (the workspace of post-activations) and
 * moves the same bytes.  At v = 0 the table gives what torch's backward gives: relu 0, lrelu 0.01, selu L A, elu 1.
 * (Taken from a, the selu and lrelu derivatives are those of v <= 0 also where a positive v below 2^-149 made L v round to 0: a = 0 there.)  tanh
 * keeps the sign of a zero, tanh(-0) = -0 as in torch; a layer's accumulator starts at +0, so its pre-activations are never -0 anyway.
 *
 * Non-finite values behave as in torch: NaN propagates through every activation (relu(NaN) is NaN, not 0); relu(-inf) = 0, lrelu(-inf) = -inf,
 * tanh(+-inf) = +-1, sigmoid(-inf) = 0, sigmoid(+inf) = 1, selu(-inf) = -L A, elu(-inf) = -1; +inf stays +inf through elu, selu, relu, lrelu and
 * identity.  The padded columns of a hidden layer are 0 whatever the activation (sigmoid(0) = 0.5 is not stored there): the next layer's K padding
 * relies on the zero.
 *
 * Error bounds against float64, u = 2^-24.  exp is dm_exp (include/go2sim_detmath.h), held below 2 ulp of its result by tests/test_detmath.py: a
 * relative error below 4 u.  None of the forms overflows: every argument of exp is <= 0, so e is in [0, 1] (0 beyond -87, where the true value is
 * below 2^-125).  The division is IEEE's, correctly rounded.  Derived as ELU_ABS is in tests/policy_ref.py, not measured:
 *   elu       v > 0: exact.  v <= 0: 4 u                  (4 u e <= 4 u from exp; the rounding of "- 1", at most u / 2, only where e < 1/2: 2.5 u there)
 *   selu      v > 0: 2 u |a| + 2^-149                     (L rounded to float32: u |a|; the product's rounding: u |a|, or half the subnormal spacing
 *                                                          2^-149 where the product lies below 2^-126)
 *             v <= 0: 10 u                                (exp(v) - 1 within 4 u as for elu, times L A = 1.758...: 7.04 u; L A rounded to float32:
 *                                                          1.76 u; the product's rounding, |a| < 2: u)
 *   relu      exact
 *   lrelu     v > 0: exact.  v <= 0: 2 u |a| + 2^-149     (0.01 rounded to float32, then the product's rounding, as for selu)
 *   tanh      5 u                                         (with E = exp(-2 |v|) and T = (1 - E) / (1 + E): dT / dE = -2 / (1 + E)^2, so the 4 u E of
 *                                                          exp arrive as 8 u E / (1 + E)^2 <= 2 u; the rounding of 1 - e, u / 2, divided by 1 + E >= 1;
 *                                                          the rounding of 1 + e in [1, 2], u, times T / (1 + E) <= 1; the quotient's rounding, u / 2:
 *                                                          4 u to first order, the fifth covers the products of these terms)
 *   sigmoid   3 u                                         (with E = exp(-|v|), v >= 0: S = 1 / (1 + E): 4 u E / (1 + E)^2 <= u from exp, the rounding
 *                                                          of 1 + e times S / (1 + E) <= 1: u, the quotient's in [1/2, 1]: u / 2.  v < 0: S = E / (1 + E)
 *                                                          <= 1/2: u + u / 2 + u / 4.  2.5 u to first order)
 *   identity  exact
 * tanh and sigmoid are bounded in absolute terms only: near v = 0 tanh loses relative accuracy to the cancellation in 1 - e (|a - tanh v| stays below
 * 5 u, a fraction of v's own rounding at unit scale).  tests/test_act_gpu.py holds the library to these numbers element by element; whole networks and
 * updates are held to the project's constants C_MLP, C_GRAD and C_UPD (include/go2sim_policy.h, include/go2sim_train.h) against float64 with the
 * matching module.
 */
#ifndef GO2SIM_ACTIVATION_H
#define GO2SIM_ACTIVATION_H

#include "go2sim.h"
#include "go2sim_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

enum go2sim_act {
  GO2SIM_ACT_ELU = 0,
  GO2SIM_ACT_SELU,
  GO2SIM_ACT_RELU,
  GO2SIM_ACT_LRELU,
  GO2SIM_ACT_TANH,
  GO2SIM_ACT_SIGMOID,
  GO2SIM_ACT_IDENTITY,
  GO2SIM_ACT_COUNT
};

/* Sets the activation of the hidden layers of `h`: a field of the handle on the host, no launch, nothing waits.  GO2SIM_E_BADARG for a NULL handle
 * or act outside 0 .. GO2SIM_ACT_COUNT - 1 (the handle is unchanged then).  Call it before the network's first launch: every launch, of inference
 * and of the updates that were created on this handle alike, reads the field when it is enqueued, so work already enqueued keeps the value it was
 * enqueued with, and a step captured into a graph keeps the value it was captured with. */
int go2sim_act_set(go2sim_mlp_t* h, int act);
/* *out = the handle's activation.  GO2SIM_E_BADARG for a NULL handle or a NULL out. */
int go2sim_act_get(const go2sim_mlp_t* h, int* out);

#ifdef __cplusplus
}
#endif
#endif
