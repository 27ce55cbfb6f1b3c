// K23: the random part of WalkingTask.reset (walking_task.py:353-392 with generate_step_sequence :137-182) drawn on the
// device into the reset-record ring that K10 / K13 read, for all N environments in one launch and without a host
// read-back:
//   oly_a3_reset_draw    base[n] += pool_count[n]; pool_count[n] = 0; slot j of environment n = record(seed, n, base[n] + j)
// record(seed, n, k) is a pure function: Philox4x32-10 with key (seed lo32, seed hi32) and counter (k lo32, k hi32, n, 0)
// gives r0..r3, and
//   mode  = STANDING if r0 < 858993459 (floor(0.2 * 2^32)) else FORWARD        p = [0.2, 0, 0, 0.8]
//   phase = period / 2 if bit 31 of r1 else 0;  step height +h if bit 30 of r1 else -h;  c = 2 + bit 29 of r1
//   first = 0.095 + (0.105 - 0.095) * u,  u = ((r2 >> 5) * 2^26 + (r3 >> 6)) * 2^-53          numpy's uniform
// and the local step sequence follows with vecstep.draw_reset_records' arithmetic (x by repeated x + 0.3, y alternating,
// z accumulating the step height for i > c).  Nothing is stored between calls but base[N].
// One workgroup per environment: its threads read base[n] / pool_count[n], meet at a barrier, and thread 0 writes them
// back, so no other workgroup reads what this one writes.  One lane per 8-byte word of the ring (a record is 82 words:
// two header words, then seq[20][4]): a wave's 64 stores cover 512 consecutive bytes.  Every lane runs the generator for
// its word's record and rebuilds the one value it stores (at most 19 additions): no loads beyond the two cursors, and
// the generator's 32-bit multiplies, not HBM, bound the launch (1.2 - 1.5 TB/s of stores at 32 records and more per
// environment).
#include "oly_common.h"

namespace {
constexpr int THREADS = 256;
constexpr int REC_WORDS = (int)(sizeof(oly_a3_reset_record) / 8);   // 82
static_assert(sizeof(oly_a3_reset_record) == 656 && REC_WORDS == 82, "oly_a3_reset_record is 82 eight-byte words");
static_assert(OLY_MAX_SEQ == 20, "generate_step_sequence makes 20 steps");

struct Draw {
  uint32_t r[4];
};

__device__ __forceinline__ Draw philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Draw{{c0, c1, c2, c3}};
}

union Word {
  double d;
  int32_t i[2];
};

// word w (0 .. 81) of record(seed, n, k)
__device__ __forceinline__ Word record_word(uint64_t seed, int n, uint64_t k, int w, double h, int period) {
  const Draw d = philox4x32_10((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)n, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const bool fwd = d.r[0] >= 858993459u;
  const int phase = (d.r[1] >> 31) ? period / 2 : 0;
  Word out;
  if (w == 0) { out.i[0] = fwd ? OLY_MODE_FORWARD : OLY_MODE_STANDING; out.i[1] = phase; return out; }
  if (w == 1) { out.i[0] = fwd ? OLY_MAX_SEQ : 1; out.i[1] = 0; return out; }
  const int i = (w - 2) >> 2, col = (w - 2) & 3;
  const bool half = (double)phase == 0.5 * (double)period;      // draw_reset_records' test, on the integer phase
  double v = 0.0;
  if (i == 0) {
    if (col == 1) {
      const double u = ((double)(d.r[2] >> 5) * 67108864.0 + (double)(d.r[3] >> 6)) * (1.0 / 9007199254740992.0);
      const double first = 0.095 + (0.105 - 0.095) * u;
      v = half ? -1 * first : 1 * first;
    }
  } else if (fwd) {
    if (col == 0) {
      for (int s = 1; s <= i; ++s) v = v + 0.3;
    } else if (col == 1) {
      v = half ? -0.15 : 0.15;
      if (i & 1) v = v * -1;
    } else if (col == 2) {
      const double step = ((d.r[1] >> 30) & 1u) ? h : -h;
      const int c = 2 + (int)((d.r[1] >> 29) & 1u);
      for (int s = c + 1; s <= i; ++s) v = v + step;
    }
  }
  out.d = v;
  return out;
}

__global__ __launch_bounds__(THREADS) void a3_reset_draw_kernel(oly_a3_reset_record* pool, int pool_depth, uint64_t seed,
                                                                int64_t* base, int32_t* pool_count, double h, int period) {
  const int n = blockIdx.x;
  int64_t b = base[n];
  if (pool_count) {
    b += pool_count[n];
    __syncthreads();                                  // every thread of the only workgroup that reads the two has read them
    if (threadIdx.x == 0) { base[n] = b; pool_count[n] = 0; }
  }
  int2* ring = reinterpret_cast<int2*>(pool + (size_t)n * pool_depth);
  const int words = pool_depth * REC_WORDS;
  for (int e = threadIdx.x; e < words; e += THREADS) {
    const int j = e / REC_WORDS, w = e - j * REC_WORDS;
    const Word x = record_word(seed, n, (uint64_t)b + (uint64_t)j, w, h, period);
    ring[e] = make_int2(x.i[0], x.i[1]);
  }
}
}  // namespace

extern "C" int oly_a3_reset_draw(oly_ctx* ctx, oly_a3_reset_record* pool, int N, int pool_depth, uint64_t seed, int64_t* base,
                                 int32_t* pool_count, double step_height_abs, int period, oly_stream stream) {
  if (!ctx) return OLY_EINVAL;
  if (!pool || !base) OLY_FAIL(ctx, OLY_EINVAL, "oly_a3_reset_draw: NULL pool / base");
  if (N <= 0 || pool_depth <= 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_a3_reset_draw: N = %d, pool_depth = %d", N, pool_depth);
  if (reinterpret_cast<uintptr_t>(pool) % 8 != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_a3_reset_draw: pool is not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(base) % 8 != 0) OLY_FAIL(ctx, OLY_EINVAL, "oly_a3_reset_draw: base is not 8-byte aligned");
  if (pool_depth > INT32_MAX / REC_WORDS)
    OLY_FAIL(ctx, OLY_EINVAL, "oly_a3_reset_draw: pool_depth = %d, at most %d", pool_depth, INT32_MAX / REC_WORDS);
  if (period < 0 || !(step_height_abs >= 0.0))
    OLY_FAIL(ctx, OLY_EINVAL, "oly_a3_reset_draw: period = %d, step_height_abs = %g", period, step_height_abs);
  hipLaunchKernelGGL(a3_reset_draw_kernel, dim3((unsigned)N), dim3(THREADS), 0, oly_s(stream), pool, pool_depth, seed, base,
                     pool_count, step_height_abs, period);
  OLY_LAUNCH_CHECK(ctx, "a3_reset_draw_kernel");
  return OLY_OK;
}
