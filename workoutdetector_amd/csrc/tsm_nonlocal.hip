// The embedded-Gaussian non-local block's two kernels (TSM's NL3DWrapper / NONLocalBlock3D around layer2.{0,2} and
// layer3.{0,2,4}): the 2x2 max-pool of the phi | g channels and the fused attention y = softmax(theta . phi^T) g.
// fp32 only; the block's 1x1 convs run on conv_igemm like every other conv of the engine.
#include "tsm_device.h"
#include "tsm_host_util.h"   // pool2_size, tiles_over: the launchers' sizes are the ones tests/nonlocal_host.cpp checks

#include <cmath>

namespace tsm {

// ---------------------------------------------------------------------------------------------
// maxpool2x2_kernel: MaxPool3d((1, 2, 2)) of an NHWC tensor = a 2x2 max-pool at stride 2, floor mode, no padding (a last odd
// row / column is dropped), over the channel range [c0, c0 + 4 * c4) of rows `ld` floats apart, into a DENSE
// [n, hi / 2, wi / 2, 4 * c4] tensor.  One thread per 16-byte channel quad of an output pixel; the four source pixels of
// an output are always inside the frame (2 oy + 1 <= hi - 1), so there is no bounds test beyond the grid-stride loop's.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) maxpool2x2_kernel(const float *__restrict__ x, float *__restrict__ y, int n, int hi, int wi,
                                                         int ho, int wo, int64_t ld, int c0, int c4) {
  const int64_t total = (int64_t)n * ho * wo * c4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int g = (int)(i % c4);
    int64_t pix = i / c4;
    const int ox = (int)(pix % wo);
    pix /= wo;
    const int oy = (int)(pix % ho);
    const int64_t f = pix / ho;
    const float *p = x + ((f * hi + 2 * oy) * wi + 2 * ox) * ld + c0 + 4 * g;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(p), b = *reinterpret_cast<const f32x4 *>(p + ld);
    const f32x4 c = *reinterpret_cast<const f32x4 *>(p + wi * ld), d = *reinterpret_cast<const f32x4 *>(p + (wi + 1) * ld);
    f32x4 m;
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = fmaxf(fmaxf(a[e], b[e]), fmaxf(c[e], d[e]));
    *reinterpret_cast<f32x4 *>(y + i * 4) = m;
  }
}

hipError_t launch_maxpool2x2(const float *x, int64_t ld, int c0, int c, float *y, int n, int hi, int wi, hipStream_t s) {
  if (!x || !y || n <= 0 || hi < 2 || wi < 2 || c <= 0 || c0 < 0 || c % 4 != 0 || c0 % 4 != 0 || ld % 4 != 0 || ld < c0 + c)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) return hipErrorInvalidValue;
  const int ho = tsm_host::pool2_size(hi), wo = tsm_host::pool2_size(wi);
  const int64_t total = (int64_t)n * ho * wo * (c / 4);
  TSM_KLAUNCH(maxpool2x2_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, s, x, y, n, hi, wi, ho, wo, ld, c0, c / 4);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// nonlocal_attn_kernel<D>: y[b, i, :] = sum_j softmax_j(q[b, i, :] . k[b, j, :]) v[b, j, :] for i < nq, j < nk, D channels; no
// scale factor.  Rows of q are ldq floats apart, of k and v ldkv, of y ldy; clip b's rows follow clip b - 1's.
//
// One workgroup of four waves per (64-query tile, clip), one shot.  It walks the keys in tiles of 64 with an online softmax:
// nothing anywhere has a size proportional to nq * nk.  Per key tile:
//   S  the 64 x 64 scores as 2 x 2 waves of one 32 x 32 MFMA tile, exactly as cosine_dist_kernel computes its tile: per 32
//      channels both panels go global -> registers -> LDS rows de-interleaved [even x16 | odd x16], the next step's loads in
//      flight under this step's 16 v_mfma_f32_32x32x2_f32 (operand order: tsm_igemm.hip).  Query rows >= nq and key rows >= nk
//      are not read (they stage zeros).
//   M  the scores go to LDS, keys >= nk as -inf.  Four lanes per query row: tile maximum, m' = max(m, tile maximum),
//      p = exp(s - m') written over the scores (exactly 0 for the masked keys), l = l * exp(m - m') + sum p.  A key tile always
//      holds a real key, so m' is finite and (-inf) - (-inf) never arises; the first tile's rescale factor is exp(-inf) = 0.
//   R  every wave rescales its output accumulators by exp(m - m').
//   PV O += P V per 128-channel chunk of V and per 32 keys: the V rows go global -> LDS as they are (keys >= nk as zeros, a
//      half tile without a real key is skipped), the B operand is read straight along the channels (lane = channel, the two
//      lane halves the two keys of the step), the A operand is P.  Wave w owns channels 32 w .. 32 w + 31 of every chunk
//      (D / 4 output columns), both 32-row halves: D / 128 * 2 accumulator tiles, 64 / 128 registers per lane.
// Epilogue: y = O / l for the rows < nq.
//
// Summation order: every output element is one chain over the key tiles in ascending order, inside a tile over the keys in
// ascending order; the row sum l likewise (16-key quarters, combined (q0 + q1) + (q2 + q3)).  The order depends on (i, nk) only:
// not on the clip, the grid or the number of clips.  No atomics.
// ---------------------------------------------------------------------------------------------
constexpr int kAttnTile = 64;    // queries per workgroup = keys per step
constexpr int kAttnPld = 66;     // score / probability row stride: lane l31 and half h read bank 2 l31 + h (+ 2 e)
constexpr int kAttnVc = 128;     // channels of V per staging pass
constexpr int kAttnVld = 160;    // V row stride: the two lane halves (keys 2 e, 2 e + 1) are 32 banks apart

template <int D>
__global__ void __launch_bounds__(256) nonlocal_attn_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                            const float *__restrict__ v, float *__restrict__ y, int nq, int nk,
                                                            int64_t ldq, int64_t ldkv, int64_t ldy) {
  static_assert(D % kAttnVc == 0 && D % kBK == 0, "D is a multiple of the V chunk and of the K-step");
  constexpr int NC = D / kAttnVc;
  __shared__ __attribute__((aligned(16))) float panels[2 * kAttnTile * kLds];   // Q panel | K panel of one 32-channel step
  __shared__ __attribute__((aligned(16))) float ps[kAttnTile * kAttnPld];       // scores, then probabilities
  __shared__ __attribute__((aligned(16))) float vs[32 * kAttnVld];              // 32 keys x 128 channels of V
  __shared__ float row_m[kAttnTile], row_l[kAttnTile], row_a[kAttnTile];        // running maximum, running sum, this tile's rescale
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int half = lane >> 5, l31 = lane & 31;
  const int lrow = tid >> 3, lk = (tid & 7) * 4;   // panel loader: rows lrow and lrow + 32, channels lk .. lk + 3 of the step
  const int64_t b = blockIdx.y, i0 = (int64_t)blockIdx.x * kAttnTile;
  const float *qb = q + b * nq * ldq, *kb = k + b * nk * ldkv, *vb = v + b * nk * ldkv;
  float *yb = y + b * nq * ldy;

  if (tid < kAttnTile) {
    row_m[tid] = -INFINITY;
    row_l[tid] = 0.f;
  }
  f32x16 o[NC][2];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[c][rh][e] = 0.f;

  for (int j0 = 0; j0 < nk; j0 += kAttnTile) {
    // ---- S: scores of queries i0 .. i0 + 63 against keys j0 .. j0 + 63
    const float *src[4];   // Q rows lrow, lrow + 32; K rows lrow, lrow + 32 (null: the row does not exist)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t r = (t < 2 ? i0 : (int64_t)j0) + lrow + 32 * (t & 1);
      src[t] = t < 2 ? (r < nq ? qb + r * ldq + lk : nullptr) : (r < nk ? kb + r * ldkv + lk : nullptr);
    }
    f32x4 regs[4];
    auto fetch = [&](int kt) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        regs[t] = src[t] ? *reinterpret_cast<const f32x4 *>(src[t] + kt * kBK) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    fetch(0);
    for (int kt = 0; kt < D / kBK; ++kt) {
      __syncthreads();   // the previous step's fragments have been read (first step: the previous key tile is done with its LDS)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float *row = panels + ((t >> 1) * kAttnTile + lrow + 32 * (t & 1)) * kLds + (lk >> 1);
        *reinterpret_cast<f32x2 *>(row) = f32x2{regs[t][0], regs[t][2]};        // even channels
        *reinterpret_cast<f32x2 *>(row + 16) = f32x2{regs[t][1], regs[t][3]};   // odd channels
      }
      __syncthreads();
      if (kt + 1 < D / kBK) fetch(kt + 1);
      const float *As = panels + (wm * 32 + l31) * kLds + half * 16;
      const float *Bs = panels + (kAttnTile + wn * 32 + l31) * kLds + half * 16;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(As + g4 * 4);
        const f32x4 bb = *reinterpret_cast<const f32x4 *>(Bs + g4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bb[e], acc, 0, 0, 0);
      }
    }
    // ---- M: scores to LDS (keys past nk as -inf), then the row statistics
    {
      const int col = wn * 32 + l31;
      const bool real = j0 + col < nk;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = (r & 3) + 8 * (r >> 2) + 4 * half;
        ps[(wm * 32 + il) * kAttnPld + col] = real ? acc[r] : -INFINITY;
      }
    }
    __syncthreads();
    {
      const int row = tid >> 2, qd = tid & 3;   // four neighbouring lanes per row, 16 keys each
      float *pr = ps + row * kAttnPld + qd * 16;
      float mx = pr[0];
#pragma unroll
      for (int c = 1; c < 16; ++c) mx = fmaxf(mx, pr[c]);
      mx = fmaxf(mx, __shfl_xor(mx, 1));
      mx = fmaxf(mx, __shfl_xor(mx, 2));
      const float m_old = row_m[row], l_old = row_l[row];
      const float m_new = fmaxf(m_old, mx);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const float p = expf(pr[c] - m_new);
        pr[c] = p;
        sum += p;
      }
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      const float alpha = expf(m_old - m_new);
      if (qd == 0) {
        row_m[row] = m_new;
        row_l[row] = l_old * alpha + sum;
        row_a[row] = alpha;
      }
    }
    __syncthreads();
    // ---- R: rescale the output accumulators
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float alpha = row_a[rh * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
        for (int c = 0; c < NC; ++c) o[c][rh][r] *= alpha;
      }
    // ---- PV
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int jh = 0; jh < 2; ++jh) {
        const int jbase = j0 + jh * 32;
        if (jbase >= nk) continue;   // (uniform over the workgroup) no real key in this half: its probabilities are all 0
        __syncthreads();             // the previous pass's V rows have been read
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int idx = tid + 256 * t, r = idx >> 5, c4 = idx & 31;
          const int64_t key = jbase + r;
          const f32x4 val = key < nk ? *reinterpret_cast<const f32x4 *>(vb + key * ldkv + c * kAttnVc + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<f32x4 *>(vs + r * kAttnVld + c4 * 4) = val;
        }
        __syncthreads();
        const float *Pa = ps + l31 * kAttnPld + jh * 32 + half;
        const float *Vb = vs + half * kAttnVld + wave * 32 + l31;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float bv = Vb[2 * e * kAttnVld];
#pragma unroll
          for (int rh = 0; rh < 2; ++rh)
            o[c][rh] = __builtin_amdgcn_mfma_f32_32x32x2f32(Pa[rh * 32 * kAttnPld + 2 * e], bv, o[c][rh], 0, 0, 0);
        }
      }
    }
  }
  // ---- epilogue (row_l is final since the barrier behind the last tile's M)
#pragma unroll
  for (int rh = 0; rh < 2; ++rh)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rh * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int64_t i = i0 + row;
      if (i >= nq) continue;
      const float inv = 1.f / row_l[row];
#pragma unroll
      for (int c = 0; c < NC; ++c) yb[i * ldy + c * kAttnVc + wave * 32 + l31] = o[c][rh][r] * inv;
    }
}

hipError_t launch_nonlocal_attention(const float *q, int64_t ldq, const float *k, const float *v, int64_t ldkv, float *y,
                                     int64_t ldy, int n_clips, int nq, int nk, int d, hipStream_t s) {
  if (d != 256 && d != 512) return hipErrorNotSupported;
  // (nk: the kernel's key-tile counter j0 is an int that steps past nk by up to one tile)
  if (!q || !k || !v || !y || n_clips <= 0 || n_clips > 65535 || nq <= 0 || nk <= 0 || nk > INT32_MAX - kAttnTile || ldq < d || ldkv < d || ldy < d ||
      ldq % 4 != 0 || ldkv % 4 != 0)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) & 15u) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tsm_host::tiles_over(nq, kAttnTile), (unsigned)n_clips);
  if (d == 256) TSM_KLAUNCH(nonlocal_attn_kernel<256>, grid, dim3(256), 0, s, q, k, v, y, nq, nk, ldq, ldkv, ldy);
  else TSM_KLAUNCH(nonlocal_attn_kernel<512>, grid, dim3(256), 0, s, q, k, v, y, nq, nk, ldq, ldkv, ldy);
  return hipGetLastError();
}

}  // namespace tsm
