/* go2sim_state.h -- exact snapshots of an env handle: save, load, bit-identical continuation.
 *
 * An env step is a pure function of the handle's state, the actions and (seed, env, step, purpose).  A record written by go2sim_state_save and
 * put back by go2sim_state_load into a handle built from the same model blob, configuration, n_envs and seed makes that handle continue bit for
 * bit as the saved one did -- under either executor (step graph or plain launches) and with any team sizes, which are not part of the state.
 *
 * Conventions follow go2sim_tiles.h: extern "C", int status (0 = ok, GO2SIM_E_*), work is ordered on the given stream.  Product library only:
 * the CPU oracle has no twin.  The handle's layout stays private to csrc/go2sim.hip; csrc/go2sim_state.hip works over go2sim_state_view.
 *
 * The record is device memory, 16-byte aligned: a header of GO2SIM_STATE_HDR_WORDS uint32 words, then the body.
 *
 * Header words (GO2SIM_STATE_W_*):
 *   MAGIC, VERSION, N_ENVS
 *   NQ, ND, NL, NG, NA, NM, NOBS_MAX, NPRIV_MAX, NREW, MAX_CONTACTS, MAX_ROWS    the layout constants of the build
 *   F_ROWS, I_ROWS, AF_STRIDE, AI_STRIDE, GLOB_BYTES, ACC_BYTES                   rows of the two SoA pools, record strides of the two AoS pools
 *   F_CARRIED, I_CARRIED, AF_CARRIED, AI_CARRIED                                  what the body carries of each pool: rows, rows, 16-byte chunks per
 *                                                                                 env, 16-byte chunks per env
 *   SEED (2 words), MODEL_DIGEST (2), CFG_DIGEST (2), BYTES (2)                   64-bit values, low word first
 *   STEP_COUNT, ACTION_WRITE_IDX                                                  the host scalars that feed the step kernels' arguments
 * The digests are FNV-1a (64 bit) over the model blob as handed to go2sim_create -- continued, on a handle with a heightfield, over the field in
 * metres as go2sim_set_terrain[_f32] installed it with its shape, cell size and origin -- and over the configuration as go2sim_env_configure
 * stored it (the doubles, the floats, the ints; the tile grid and the well centres are configuration).  What the host changes in the model tables
 * after create through go2sim_set_friction / go2sim_set_dof_gains is in neither digest: the caller repeats those calls on the loading handle.  A tiny kernel writes the header from kernel arguments.  The words below GO2SIM_STATE_W_CHECKED are
 * compared by go2sim_state_load, on the device, against those of the loading handle before anything is written.
 *
 * Body, each part starting on a 16-byte boundary (the bytes up to it are zero), in this order: the env globals (go2sim_env_globals_t), the step's
 * accumulator, the carried rows of the SoA float pool [F_CARRIED][n_envs], those of the SoA int pool [I_CARRIED][n_envs], the carried chunks of
 * the AoS float records [n_envs][AF_CARRIED][4 words], those of the AoS int records [n_envs][AI_CARRIED][4 words]; then, on a handle configured
 * with GO2SIM_IC_ENGINE_BATCH_GAIN, the engine gains (kp, kv) of the twelve motor dofs as the device model tables hold them: with that mode
 * k_env_engine_gains rewrites them after every step that had a reset, and the next step's dynamics, solve and control-force rewards read them, so
 * they are state although they live in the model.  load writes them into both tables (Model and the compact ModelS).  No other kernel writes a
 * model table.
 *
 * The carried set.  A field is carried when a step may read it before it writes it, or when the field API (go2sim_get_field) shows values an
 * earlier step left in it; the flag in the four field tables of csrc/go2sim.hip is the one place that says which (DESIGN.md "Env state" lists
 * them with the reason for each dropped one).  SoA pools are carried by rows.  AoS records are carried by 16-byte chunks: a chunk is carried when
 * a word of a carried field lies in it, so that both sides of the copy are whole 16-byte accesses (a dropped field gives up to three words at each
 * end to its neighbours' chunks; load writes them back with the values they were saved with).  GO2SIM_STATE_WHOLE=1, read by go2sim_create,
 * makes the handle carry every row and every chunk -- the whole-pool form, correct by construction, kept as the yardstick of the carried one; its
 * records have other F_CARRIED ... AI_CARRIED words and are refused by a handle of the other form.  Scratch (the GJK / EPA polytope records, the
 * solver's overflow blocks, the heaviest-first dispatch records, timing state) is not state.  Static inputs (model, configuration, heightfield)
 * are not state either: the caller builds the handle from them, the digests catch a mismatch of all three.
 */
#ifndef GO2SIM_STATE_H
#define GO2SIM_STATE_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_STATE_MAGIC 0x54533247
#define GO2SIM_STATE_VERSION 1
#define GO2SIM_STATE_HDR_WORDS 64
#define GO2SIM_STATE_N_POOLS 4
#define GO2SIM_STATE_MAX_SPANS 16
#define GO2SIM_STATE_MAX_GAIN_WORDS 24

enum go2sim_state_word {
  GO2SIM_STATE_W_MAGIC = 0, GO2SIM_STATE_W_VERSION, GO2SIM_STATE_W_N_ENVS,
  GO2SIM_STATE_W_NQ, GO2SIM_STATE_W_ND, GO2SIM_STATE_W_NL, GO2SIM_STATE_W_NG, GO2SIM_STATE_W_NA, GO2SIM_STATE_W_NM, GO2SIM_STATE_W_NOBS_MAX,
  GO2SIM_STATE_W_NPRIV_MAX, GO2SIM_STATE_W_NREW, GO2SIM_STATE_W_MAX_CONTACTS, GO2SIM_STATE_W_MAX_ROWS,
  GO2SIM_STATE_W_F_ROWS, GO2SIM_STATE_W_I_ROWS, GO2SIM_STATE_W_AF_STRIDE, GO2SIM_STATE_W_AI_STRIDE, GO2SIM_STATE_W_GLOB_BYTES, GO2SIM_STATE_W_ACC_BYTES,
  GO2SIM_STATE_W_F_CARRIED, GO2SIM_STATE_W_I_CARRIED, GO2SIM_STATE_W_AF_CARRIED, GO2SIM_STATE_W_AI_CARRIED,
  GO2SIM_STATE_W_SEED = 24, GO2SIM_STATE_W_MODEL_DIGEST = 26, GO2SIM_STATE_W_CFG_DIGEST = 28, GO2SIM_STATE_W_BYTES = 30,
  GO2SIM_STATE_W_CHECKED = 32,
  GO2SIM_STATE_W_STEP_COUNT = 32, GO2SIM_STATE_W_ACTION_WRITE_IDX = 33
};

/* Bytes of one record for this handle's n_envs and build. */
int go2sim_state_size(go2sim_t* h, size_t* bytes);

/* Header and body into dst_dev (device memory, 16-byte aligned, `bytes` = go2sim_state_size).  Stream-ordered, no host synchronisation: the host
 * scalars travel as kernel arguments.  GO2SIM_E_BADARG for a NULL or misaligned pointer or another `bytes`. */
int go2sim_state_save(go2sim_t* h, void* dst_dev, size_t bytes, void* stream);

/* The record back into the handle.  The header is compared on the device first; the copy kernels behind it are gated on the verdict, so a refused
 * record writes nothing and the handle steps exactly as if the call had not been made.  Refused with GO2SIM_E_BADARG: another `bytes`, magic, format
 * version, n_envs, layout constant, seed, model digest or configuration digest.  Stream-ordered; the call then waits for the stream once, because
 * its status reports the verdict and the two host scalars of the record have to reach the host before the next step is enqueued. */
int go2sim_state_load(go2sim_t* h, const void* src_dev, size_t bytes, void* stream);

/* What csrc/go2sim_state.hip needs of a handle (csrc/go2sim.hip fills it): the globals and the accumulator, the four pools (SoA float, SoA int,
 * AoS float, AoS int) with their strides (rows; 16-byte chunks per record) and carried spans (of rows; of chunks), the header's words for this
 * handle (the two host scalars as they are now), device words and their pinned host twins for load's verdict, and the addresses of the host
 * scalars load applies. */
typedef struct go2sim_state_spans { int n, carried; int first[GO2SIM_STATE_MAX_SPANS], count[GO2SIM_STATE_MAX_SPANS]; } go2sim_state_spans_t;
typedef struct go2sim_state_view {
  int device, n_envs;
  void* glob; size_t glob_bytes;
  void* acc; size_t acc_bytes;
  void* pool[GO2SIM_STATE_N_POOLS];
  int stride[GO2SIM_STATE_N_POOLS];
  go2sim_state_spans_t spans[GO2SIM_STATE_N_POOLS];
  int n_gain;                         /* words of the gains part: 2 per motor dof (kp, kv) with GO2SIM_IC_ENGINE_BATCH_GAIN, else 0 */
  void* gain_dev[2][GO2SIM_STATE_MAX_GAIN_WORDS];   /* their device addresses in the two model tables: [Model | ModelS][kp0, kv0, kp1, ...] */
  uint32_t hdr[GO2SIM_STATE_HDR_WORDS];
  uint32_t* verdict_dev;              /* [4]: first differing header word + 1 (0 = accepted), step_count, action_write_idx */
  uint32_t* verdict_host;             /* [4] pinned */
  uint32_t* step_count;
  int* action_write_idx;
} go2sim_state_view_t;
int go2sim_state_view(go2sim_t* h, go2sim_state_view_t* out);

#ifdef __cplusplus
}
#endif
#endif
