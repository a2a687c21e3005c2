// go2sim_state.hip -- exact snapshots of an env handle (include/go2sim_state.h), on gfx950.  The header states the record; this file holds the
// kernels and the three entry points over go2sim_state_view, the one accessor csrc/go2sim.hip gives of its private handle layout and of the
// carried set its field tables mark.  Nothing here is on the step's path.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/go2sim_state.h"

namespace {

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { fprintf(stderr, "go2sim: HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); return GO2SIM_E_HIP; } } while (0)

constexpr int HDR = GO2SIM_STATE_HDR_WORDS, NPOOL = GO2SIM_STATE_N_POOLS, NSPAN = GO2SIM_STATE_MAX_SPANS, COPY_WG = 256, COPY_MAX_BLOCKS = 2048;
constexpr int NGAIN = GO2SIM_STATE_MAX_GAIN_WORDS;
constexpr int NSEG = 2 + 2 * NSPAN + 2 * NGAIN;   // the globals, the accumulator, the carried row spans of the two SoA pools, the engine gains word by word (load: into both model tables)
static_assert(HDR == 64, "the header kernels run one wavefront, one word per lane");

struct Header { uint32_t w[HDR]; };
// one contiguous run of 32-bit words on both sides; `pad` words behind it in the record are zeroed by pack (the bytes up to the next part)
struct Seg { const uint32_t* src; uint32_t* dst; unsigned long long words; int pad; };
struct Segs { Seg s[NSEG]; };
// the carried chunks of one AoS pool: span k is `count[k]` 16-byte chunks from chunk `first[k]` of a record, `packed[k]` chunks into the env's packed row
struct Chunks { int n, carried, stride; int first[NSPAN], count[NSPAN], packed[NSPAN]; };

// the header from kernel arguments: one word per lane, ordinary vector stores
__global__ __launch_bounds__(HDR) void k_state_header(uint32_t* __restrict__ dst, Header hdr) { dst[threadIdx.x] = hdr.w[threadIdx.x]; }

// the record's header against the loading handle's: verdict[0] = 1 + the first differing word below GO2SIM_STATE_W_CHECKED (0: accepted), then the
// record's two host scalars
__global__ __launch_bounds__(HDR) void k_state_check(const uint32_t* __restrict__ src, Header expect, uint32_t* __restrict__ verdict) {
  const int lane = threadIdx.x;
  const bool differs = lane < GO2SIM_STATE_W_CHECKED && src[lane] != expect.w[lane];
  const unsigned long long bad = __ballot(differs);
  if (lane == 0) {
    verdict[0] = bad ? (uint32_t)__ffsll(bad) : 0u;
    verdict[1] = src[GO2SIM_STATE_W_STEP_COUNT];
    verdict[2] = src[GO2SIM_STATE_W_ACTION_WRITE_IDX];
    verdict[3] = 0u;
  }
}

// The globals, the accumulator and the carried rows of the SoA pools: segment blockIdx.y, one word per lane and trip.  A span of rows is contiguous
// in the pool and in the record ([rows][n_envs] on both sides), so consecutive lanes move consecutive envs of a row.  `gate`: unpack runs behind
// k_state_check and writes nothing for a refused record.
__global__ __launch_bounds__(COPY_WG) void k_state_copy_words(Segs p, const uint32_t* __restrict__ gate) {
  if (gate && gate[0] != 0u) return;
  const Seg g = p.s[blockIdx.y];
  const size_t n = g.words;
  for (size_t i = (size_t)blockIdx.x * COPY_WG + threadIdx.x; i < n; i += (size_t)gridDim.x * COPY_WG) g.dst[i] = g.src[i];
  if (blockIdx.x == 0 && (int)threadIdx.x < g.pad) g.dst[n + threadIdx.x] = 0u;
}

// The carried chunks of an AoS pool between the records [n_envs][stride] and the packed rows [n_envs][carried], 16 bytes per lane and trip on both
// sides: lane i of the grid owns packed chunk i, finds its span (a handful, searched in order) and with it the chunk of the env's record.
// Consecutive lanes move consecutive chunks of a span, whole 64-byte-aligned records are never read beyond their carried spans.
__global__ __launch_bounds__(COPY_WG) void k_state_copy_chunks(uint4* __restrict__ pool, uint4* __restrict__ rec, Chunks c, unsigned long long total, int to_record,
                                                                const uint32_t* __restrict__ gate) {
  if (gate && gate[0] != 0u) return;
  for (size_t i = (size_t)blockIdx.x * COPY_WG + threadIdx.x; i < total; i += (size_t)gridDim.x * COPY_WG) {
    const size_t env = i / (size_t)c.carried;
    const int j = (int)(i - env * (size_t)c.carried);
    int k = 0;
    while (k + 1 < c.n && j >= c.packed[k + 1]) ++k;
    const size_t at = env * (size_t)c.stride + (size_t)(c.first[k] + (j - c.packed[k]));
    if (to_record) rec[i] = pool[at]; else pool[at] = rec[i];
  }
}

size_t pad16(size_t n) { return (n + 15) / 16 * 16; }
size_t pool_bytes(const go2sim_state_view_t& v, int k) { return (size_t)v.spans[k].carried * (k < 2 ? 4 : 16) * (size_t)v.n_envs; }
size_t record_bytes(const go2sim_state_view_t& v) {
  size_t total = (size_t)HDR * 4 + pad16(v.glob_bytes) + pad16(v.acc_bytes);
  for (int k = 0; k < NPOOL; ++k) total += pad16(pool_bytes(v, k));
  return total + pad16((size_t)v.n_gain * 4);
}
unsigned blocks_for(size_t items) {
  size_t blocks = (items + COPY_WG - 1) / COPY_WG;
  return (unsigned)(blocks < 1 ? 1 : blocks > COPY_MAX_BLOCKS ? COPY_MAX_BLOCKS : blocks);
}
// the body between the handle and the record at `rec`: one launch for the word segments, one per AoS pool
void launch_copy(const go2sim_state_view_t& v, char* rec, bool to_record, const uint32_t* gate, hipStream_t s) {
  Segs p;
  int n_seg = 0;
  size_t at = (size_t)HDR * 4, most = 0;
  auto add = [&](void* handle_side, size_t bytes, size_t pad_bytes) {
    Seg& g = p.s[n_seg++];
    g.src = (const uint32_t*)(to_record ? handle_side : (void*)(rec + at));
    g.dst = (uint32_t*)(to_record ? (void*)(rec + at) : handle_side);
    g.words = bytes / 4; g.pad = to_record ? (int)(pad_bytes / 4) : 0;
    at += bytes + pad_bytes;
    if (g.words > most) most = g.words;
  };
  add(v.glob, v.glob_bytes, pad16(v.glob_bytes) - v.glob_bytes);
  add(v.acc, v.acc_bytes, pad16(v.acc_bytes) - v.acc_bytes);
  const size_t B = (size_t)v.n_envs;
  for (int k = 0; k < 2; ++k) {
    const go2sim_state_spans_t& sp = v.spans[k];
    const size_t part = pool_bytes(v, k);
    for (int q = 0; q < sp.n; ++q)
      add((char*)v.pool[k] + (size_t)sp.first[q] * B * 4, (size_t)sp.count[q] * B * 4, q + 1 == sp.n ? pad16(part) - part : 0);
    if (sp.n == 0) at += pad16(part) - part;
  }
  {   // the engine gains, the last part of the record: one word per segment (they are scattered over the model tables' dof records)
    const size_t body_end = at;
    at = record_bytes(v) - pad16((size_t)v.n_gain * 4);
    for (int k = 0; k < v.n_gain; ++k) {
      const size_t here = at;
      add(v.gain_dev[0][k], 4, 0);
      if (!to_record) { at = here; add(v.gain_dev[1][k], 4, 0); }
    }
    if (to_record && v.n_gain > 0) p.s[n_seg - 1].pad = (int)((pad16((size_t)v.n_gain * 4) - (size_t)v.n_gain * 4) / 4);
    at = body_end;
  }
  hipLaunchKernelGGL(k_state_copy_words, dim3(blocks_for(most), n_seg), dim3(COPY_WG), 0, s, p, gate);
  for (int k = 2; k < NPOOL; ++k) {
    const go2sim_state_spans_t& sp = v.spans[k];
    if (sp.carried == 0) continue;
    Chunks c;
    c.n = sp.n; c.carried = sp.carried; c.stride = v.stride[k];
    for (int q = 0, packed = 0; q < NSPAN; ++q) {
      c.first[q] = q < sp.n ? sp.first[q] : 0; c.count[q] = q < sp.n ? sp.count[q] : 0; c.packed[q] = packed;
      packed += c.count[q];
    }
    const size_t total = (size_t)sp.carried * B;
    hipLaunchKernelGGL(k_state_copy_chunks, dim3(blocks_for(total)), dim3(COPY_WG), 0, s, (uint4*)v.pool[k], (uint4*)(rec + at), c, (unsigned long long)total,
                       to_record ? 1 : 0, gate);
    at += pad16(pool_bytes(v, k));
  }
}
const char* word_name(int w) {
  if (w == GO2SIM_STATE_W_MAGIC) return "magic";
  if (w == GO2SIM_STATE_W_VERSION) return "format version";
  if (w == GO2SIM_STATE_W_N_ENVS) return "n_envs";
  if (w < GO2SIM_STATE_W_SEED) return "layout constant";
  if (w < GO2SIM_STATE_W_MODEL_DIGEST) return "seed";
  if (w < GO2SIM_STATE_W_CFG_DIGEST) return "model digest";
  if (w < GO2SIM_STATE_W_BYTES) return "configuration digest";
  return "record size";
}

}  // namespace

extern "C" {

int go2sim_state_size(go2sim_t* h, size_t* bytes) {
  go2sim_state_view_t v;
  if (!bytes || go2sim_state_view(h, &v) != GO2SIM_E_OK) return GO2SIM_E_BADARG;
  *bytes = record_bytes(v);
  return GO2SIM_E_OK;
}

int go2sim_state_save(go2sim_t* h, void* dst_dev, size_t bytes, void* stream) {
  go2sim_state_view_t v;
  if (!dst_dev || ((uintptr_t)dst_dev & 15) || go2sim_state_view(h, &v) != GO2SIM_E_OK || bytes != record_bytes(v)) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(v.device));
  Header hdr;
  for (int k = 0; k < HDR; ++k) hdr.w[k] = v.hdr[k];
  hipLaunchKernelGGL(k_state_header, dim3(1), dim3(HDR), 0, s, (uint32_t*)dst_dev, hdr);
  launch_copy(v, (char*)dst_dev, true, nullptr, s);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_state_load(go2sim_t* h, const void* src_dev, size_t bytes, void* stream) {
  go2sim_state_view_t v;
  if (!src_dev || ((uintptr_t)src_dev & 15) || go2sim_state_view(h, &v) != GO2SIM_E_OK) return GO2SIM_E_BADARG;
  if (bytes != record_bytes(v)) {
    fprintf(stderr, "go2sim_state_load: refused, the record has %zu bytes and this handle's records have %zu\n", bytes, record_bytes(v));
    return GO2SIM_E_BADARG;
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(v.device));
  Header expect;
  for (int k = 0; k < HDR; ++k) expect.w[k] = v.hdr[k];
  hipLaunchKernelGGL(k_state_check, dim3(1), dim3(HDR), 0, s, (const uint32_t*)src_dev, expect, v.verdict_dev);
  launch_copy(v, (char*)src_dev, false, v.verdict_dev, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(v.verdict_host, v.verdict_dev, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (v.verdict_host[0] != 0u) {
    fprintf(stderr, "go2sim_state_load: refused, the record's %s differs from this handle's (header word %u)\n", word_name((int)v.verdict_host[0] - 1),
            v.verdict_host[0] - 1);
    return GO2SIM_E_BADARG;
  }
  *v.step_count = v.verdict_host[1];
  *v.action_write_idx = (int)v.verdict_host[2];
  return GO2SIM_E_OK;
}

}  // extern "C"
