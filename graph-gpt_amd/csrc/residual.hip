// libgget_hip.so - the residual add as its own kernel, for models with LayerScale, DropPath or MLP dropout (Plan::has_res): alone, fused
// with the RMSNorm that follows it, and the two backward forms.  The RMSNorm family proper is in kernels.hip; PathDropArg, path_keep and
// the launchers' declarations are in kernels.h.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

__global__ void __launch_bounds__(256) ls_fwd_kernel(const bf16_t* __restrict__ res, const bf16_t* __restrict__ y,
                                                     const bf16_t* __restrict__ lam, bf16_t* __restrict__ out, long T, int d,
                                                     PathDrop D, ElemDropArg E) {
  const int cpr = d >> 3;
  const long total = T * cpr;
  for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < total; w += (long)gridDim.x * 256) {
    const int c = (int)(w % cpr);
    const float keep = path_keep(D, w / cpr);
    float r[8], v[8], l[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    unpack8(*reinterpret_cast<const uint4*>(res + w * 8), r);
    unpack8(*reinterpret_cast<const uint4*>(y + w * 8), v);
    if (lam) unpack8(*reinterpret_cast<const uint4*>(lam + c * 8), l);
    if (E.thresh) {   // mlp_dropout on the down projection's output (utils_graphgpt.py:79), rounded like the bf16 module does
#pragma unroll
      for (int e = 0; e < 8; ++e)
        v[e] = bf2f(f2bf(v[e] * elem_drop_mul(E, GGET_DROP_STREAM_MLP_OUT, elem_row(E, w / cpr), (unsigned)(c * 8 + e))));
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] += keep * bf2f(f2bf(l[e] * v[e]));
    *reinterpret_cast<uint4*>(out + w * 8) = pack8(r);
  }
}
// ls_fwd_kernel and the RMSNorm that always follows it (rmsnorm_fwd_kernel, kernels.hip) in one pass over the rows: the residual stream
// is written (out) and normalised (xn, rstd) without being read back - same arithmetic and rounding points as the two kernels.
// A wave owns a row at a time; NCH = 16-byte chunks per lane.
template <int NCH>
__global__ void __launch_bounds__(256) ls_rmsnorm_fwd_kernel(const bf16_t* __restrict__ res, const bf16_t* __restrict__ y,
                                                             const bf16_t* __restrict__ lam, bf16_t* __restrict__ out,
                                                             const bf16_t* __restrict__ w, bf16_t* __restrict__ xn,
                                                             float* __restrict__ rstd_out, int T, int d, float eps, PathDrop D,
                                                             ElemDropArg E) {
  const int lane = threadIdx.x & 63;
  const int nchunk = d >> 3;
  const int stride = gridDim.x * 4;
  float wv[NCH][8], lv[NCH][8];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + i * 64;
#pragma unroll
    for (int e = 0; e < 8; ++e) { wv[i][e] = 0.f; lv[i][e] = 1.f; }
    if (c < nchunk) {
      unpack8(*reinterpret_cast<const uint4*>(w + c * 8), wv[i]);
      if (lam) unpack8(*reinterpret_cast<const uint4*>(lam + c * 8), lv[i]);
    }
  }
  int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  uint4 cr[NCH], cy[NCH], nr[NCH], ny[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + i * 64;
    const bool ok = c < nchunk && row < T;
    cr[i] = ok ? *reinterpret_cast<const uint4*>(res + (size_t)row * d + c * 8) : make_uint4(0, 0, 0, 0);
    cy[i] = ok ? *reinterpret_cast<const uint4*>(y + (size_t)row * d + c * 8) : make_uint4(0, 0, 0, 0);
  }
  for (; row < T; row += stride) {
    const int nrow = row + stride;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      const bool ok = c < nchunk && nrow < T;
      nr[i] = ok ? *reinterpret_cast<const uint4*>(res + (size_t)nrow * d + c * 8) : make_uint4(0, 0, 0, 0);
      ny[i] = ok ? *reinterpret_cast<const uint4*>(y + (size_t)nrow * d + c * 8) : make_uint4(0, 0, 0, 0);
    }
    const float keep = path_keep(D, row);
    float v[NCH][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      float r[8], yv[8];
      unpack8(cr[i], r);
      unpack8(cy[i], yv);
      if (E.thresh) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          yv[e] = bf2f(f2bf(yv[e] * elem_drop_mul(E, GGET_DROP_STREAM_MLP_OUT, elem_row(E, row), (unsigned)(c * 8 + e))));
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] += keep * bf2f(f2bf(lv[i][e] * yv[e]));
      const uint4 pk = pack8(r);                    // the residual stream is a bf16 tensor: the norm sees the rounded values
      if (c < nchunk) *reinterpret_cast<uint4*>(out + (size_t)row * d + c * 8) = pk;
      unpack8(pk, v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += v[i][e] * v[i][e];
    }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / (float)d + eps);
    if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = wv[i][e] * bf2f(f2bf(v[i][e] * rstd));
        *reinterpret_cast<uint4*>(xn + (size_t)row * d + c * 8) = pack8(o);
      }
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) { cr[i] = nr[i]; cy[i] = ny[i]; }
  }
}
__global__ void __launch_bounds__(256) ls_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y,
                                                     const bf16_t* __restrict__ lam, bf16_t* __restrict__ dscaled,
                                                     float* __restrict__ dlam, int T, int d, PathDrop D, int copies,
                                                     uint64_t copy_stride, ElemDropArg E) {
  // thread = (row lane, 8-channel chunk); a block walks rows blockIdx.x*RL + lane, stride gridDim.x*RL.  The dlam partials
  // of the block's row lanes are summed through LDS and added to accumulator copy blockIdx.x % copies (GgetSegment).
  extern __shared__ float ls_lds[];   // [RL][d]
  const int CH = d >> 3, RL = 256 / CH;
  const int c = threadIdx.x % CH, rl = threadIdx.x / CH;
  const bool active = rl < RL;
  float l[8] = {1, 1, 1, 1, 1, 1, 1, 1}, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (lam && active) unpack8(*reinterpret_cast<const uint4*>(lam + c * 8), l);
  if (active) {
    for (int t = blockIdx.x * RL + rl; t < T; t += gridDim.x * RL) {
      const float keep = path_keep(D, t);
      float g[8], v[8], o[8];
      unpack8(*reinterpret_cast<const uint4*>(dy + (size_t)t * d + c * 8), g);
      unpack8(*reinterpret_cast<const uint4*>(y + (size_t)t * d + c * 8), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float em = elem_drop_mul(E, GGET_DROP_STREAM_MLP_OUT, elem_row(E, t), (unsigned)(c * 8 + e));
        o[e] = l[e] * keep * g[e] * em;
        acc[e] += keep * g[e] * bf2f(f2bf(v[e] * em));
      }
      *reinterpret_cast<uint4*>(dscaled + (size_t)t * d + c * 8) = pack8(o);
    }
  }
  if (dlam) {
    if (active) {
#pragma unroll
      for (int e = 0; e < 8; ++e) ls_lds[rl * d + c * 8 + e] = acc[e];
    }
    __syncthreads();
    float* dst = dlam + (size_t)(blockIdx.x % copies) * copy_stride;
    for (int j = threadIdx.x; j < d; j += 256) {
      float sum = 0.f;
      for (int r = 0; r < RL; ++r) sum += ls_lds[r * d + j];
      unsafeAtomicAdd(dst + j, sum);
    }
  }
}

// RMSNorm backward (rmsnorm_bwd_kernel, kernels.hip) and the LayerScale / DropPath backward that consumes its result (ls_bwd_kernel) in
// one pass over the rows: dx = dres + rstd (dy w - xhat mean(dy w xhat)) is written once and, rounded to bf16 as the separate kernel would
// read it, scaled into the gradient of the branch behind it (dsc = lam keep dx, dlam += keep dx y).  Same arithmetic as the two kernels.
template <int NCH>
__global__ void __launch_bounds__(256) rmsnorm_bwd_ls_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                             const bf16_t* __restrict__ w, const float* __restrict__ rstd_in,
                                                             const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx,
                                                             float* __restrict__ dw_accum, const bf16_t* __restrict__ y,
                                                             const bf16_t* __restrict__ lam, bf16_t* __restrict__ dsc,
                                                             float* __restrict__ dlam_accum, int T, int d, int copies,
                                                             uint64_t copy_stride, PathDrop D, ElemDropArg E) {
  extern __shared__ float red_lds[];  // [2][4][d]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = d >> 3;
  float dwp[NCH][8], dlp[NCH][8], wv[NCH][8], lv[NCH][8];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + i * 64;
#pragma unroll
    for (int e = 0; e < 8; ++e) { dwp[i][e] = 0.f; dlp[i][e] = 0.f; wv[i][e] = 0.f; lv[i][e] = 1.f; }
    if (c < nchunk) {
      unpack8(*reinterpret_cast<const uint4*>(w + c * 8), wv[i]);
      if (lam) unpack8(*reinterpret_cast<const uint4*>(lam + c * 8), lv[i]);
    }
  }
  const int stride = gridDim.x * 4;
  int row = blockIdx.x * 4 + wave;
  uint4 xr[NCH], dr[NCH], rr[NCH], yr[NCH];
  float rstd = 0.f;
  auto fetch = [&](int r) {
    rstd = rstd_in[r];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        xr[i] = *reinterpret_cast<const uint4*>(x + (size_t)r * d + c * 8);
        dr[i] = *reinterpret_cast<const uint4*>(dy + (size_t)r * d + c * 8);
        rr[i] = dres ? *reinterpret_cast<const uint4*>(dres + (size_t)r * d + c * 8) : make_uint4(0, 0, 0, 0);
        yr[i] = *reinterpret_cast<const uint4*>(y + (size_t)r * d + c * 8);
      }
    }
  };
  if (row < T) fetch(row);
  for (; row < T; row += stride) {
    const float rs = rstd;
    float xh[NCH][8], g[NCH][8], res[NCH][8], yv[NCH][8];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        float xv[8], dv[8];
        unpack8(xr[i], xv);
        unpack8(dr[i], dv);
        unpack8(rr[i], res[i]);
        unpack8(yr[i], yv[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[i][e] = xv[e] * rs;
          g[i][e] = dv[e] * wv[i][e];
          dot += g[i][e] * xh[i][e];
          dwp[i][e] += dv[e] * xh[i][e];
        }
      }
    }
    if (row + stride < T) fetch(row + stride);
    dot = wave_sum(dot) / (float)d;
    const float keep = path_keep(D, row);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        float o[8], gq[8], sc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = res[i][e] + rs * (g[i][e] - xh[i][e] * dot);
        const uint4 pk = pack8(o);
        *reinterpret_cast<uint4*>(dx + (size_t)row * d + c * 8) = pk;
        unpack8(pk, gq);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float em = elem_drop_mul(E, GGET_DROP_STREAM_MLP_OUT, elem_row(E, row), (unsigned)(c * 8 + e));
          sc[e] = lv[i][e] * keep * gq[e] * em;
          dlp[i][e] += keep * gq[e] * bf2f(f2bf(yv[i][e] * em));
        }
        *reinterpret_cast<uint4*>(dsc + (size_t)row * d + c * 8) = pack8(sc);
      }
    }
  }
  float* dl_lds = red_lds + 4 * d;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { red_lds[wave * d + c * 8 + e] = dwp[i][e]; dl_lds[wave * d + c * 8 + e] = dlp[i][e]; }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < d; j += 256) {
    const size_t off = (size_t)(blockIdx.x % copies) * copy_stride + j;
    unsafeAtomicAdd(dw_accum + off, red_lds[j] + red_lds[d + j] + red_lds[2 * d + j] + red_lds[3 * d + j]);
    if (dlam_accum) unsafeAtomicAdd(dlam_accum + off, dl_lds[j] + dl_lds[d + j] + dl_lds[2 * d + j] + dl_lds[3 * d + j]);
  }
}
// The same pass for d = 256 PCH with every lane busy and a third of the registers: lane l owns the 4 channels [256 p + 4 l, +4) of each of
// the PCH pieces of a row (8-byte loads, 512 contiguous bytes per wave instruction), norm weight and LayerScale vector stay packed, the
// residual / branch operands are unpacked where they are used, and there is no software prefetch - ~100 registers = 5 waves per SIMD keep
// 12 loads per lane in flight each instead of 2 waves x 16 (the form above: 230 registers; at d = 768 its second chunk idles half of the
// lanes).  C3 (T = 41 088, d = 768): 104 -> see profiles/r05_step_experiments.txt item 7.  Same expressions per element; the fp32 order of
// the row's dot product differs (other lane assignment), i.e. results equal the form above up to single bf16 rounding flips.
template <int PCH>
__global__ void __launch_bounds__(256) rmsnorm_bwd_ls4_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                              const bf16_t* __restrict__ w, const float* __restrict__ rstd_in,
                                                              const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx,
                                                              float* __restrict__ dw_accum, const bf16_t* __restrict__ y,
                                                              const bf16_t* __restrict__ lam, bf16_t* __restrict__ dsc,
                                                              float* __restrict__ dlam_accum, int T, int copies, uint64_t copy_stride,
                                                              PathDrop D, ElemDropArg E) {
  constexpr int d = 256 * PCH;
  extern __shared__ float red_lds[];  // [2][4][d]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto un4 = [](const uint2& v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  };
  uint2 wq[PCH], lq[PCH];
  float dwp[PCH][4], dlp[PCH][4];
#pragma unroll
  for (int p = 0; p < PCH; ++p) {
    wq[p] = *reinterpret_cast<const uint2*>(w + p * 256 + lane * 4);
    lq[p] = lam ? *reinterpret_cast<const uint2*>(lam + p * 256 + lane * 4) : make_uint2(0x3F803F80u, 0x3F803F80u);
#pragma unroll
    for (int e = 0; e < 4; ++e) { dwp[p][e] = 0.f; dlp[p][e] = 0.f; }
  }
  const int stride = gridDim.x * 4;
  // `keepv`: an empty asm the compiler must assume rewrites the packed words - the unpacked copies are recomputed where they are used
  // (one shift / and each) instead of living in registers across the loop (norm weight, LayerScale vector) or across the row's reduction
  // (x, dy): that is what takes the kernel from 149 to <= 102 registers
  auto keepv = [](uint2& v) { asm volatile("" : "+v"(v.x), "+v"(v.y)); };
  for (int row0 = blockIdx.x * 4 + wave; row0 < T; row0 += stride) {
    const int row = __builtin_amdgcn_readfirstlane(row0);     // (wave-uniform: scalar row base, 32-bit lane offsets)
    const size_t rb = (size_t)row * d;
    const bf16_t *xrow = x + rb, *dyrow = dy + rb, *yrow = y + rb, *rrow = dres ? dres + rb : nullptr;
    bf16_t *dxrow = dx + rb, *dscrow = dsc + rb;
    const unsigned lo = lane * 4;
    uint2 xr[PCH], dr[PCH], rr[PCH], yr[PCH];
#pragma unroll
    for (int p = 0; p < PCH; ++p) {
      xr[p] = *reinterpret_cast<const uint2*>(xrow + lo + p * 256);
      dr[p] = *reinterpret_cast<const uint2*>(dyrow + lo + p * 256);
    }
#pragma unroll
    for (int p = 0; p < PCH; ++p) {
      rr[p] = rrow ? *reinterpret_cast<const uint2*>(rrow + lo + p * 256) : make_uint2(0, 0);
      yr[p] = *reinterpret_cast<const uint2*>(yrow + lo + p * 256);
    }
    const float rs = rstd_in[row];
    float dot = 0.f;
#pragma unroll
    for (int p = 0; p < PCH; ++p) {
      float xv[4], dv[4], wv[4];
      keepv(wq[p]);
      un4(xr[p], xv);
      un4(dr[p], dv);
      un4(wq[p], wv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = xv[e] * rs, g = dv[e] * wv[e];
        dot += g * xh;
        dwp[p][e] += dv[e] * xh;
      }
    }
    dot = wave_sum(dot) / (float)d;
    const float keep = path_keep(D, row);
    const unsigned erow = E.thresh ? elem_row(E, row) : 0u;
#pragma unroll
    for (int p = 0; p < PCH; ++p) {
      float xv[4], dv[4], wv[4], res[4], o[4], gq[4], sc[4], lv[4], yv[4];
      keepv(xr[p]);
      keepv(dr[p]);
      keepv(wq[p]);
      keepv(lq[p]);
      un4(xr[p], xv);
      un4(dr[p], dv);
      un4(wq[p], wv);
      un4(rr[p], res);
      un4(lq[p], lv);
      un4(yr[p], yv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = xv[e] * rs, g = dv[e] * wv[e];
        o[e] = res[e] + rs * (g - xh * dot);
      }
      const uint2 pk = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
      *reinterpret_cast<uint2*>(dxrow + lo + p * 256) = pk;
      un4(pk, gq);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float em = elem_drop_mul(E, GGET_DROP_STREAM_MLP_OUT, erow, (unsigned)(p * 256 + lane * 4 + e));
        sc[e] = lv[e] * keep * gq[e] * em;
        dlp[p][e] += keep * gq[e] * bf2f(f2bf(yv[e] * em));
      }
      *reinterpret_cast<uint2*>(dscrow + lo + p * 256) = make_uint2(pack2bf(sc[0], sc[1]), pack2bf(sc[2], sc[3]));
    }
  }
  float* dl_lds = red_lds + 4 * d;
#pragma unroll
  for (int p = 0; p < PCH; ++p) {
    *reinterpret_cast<float4*>(red_lds + wave * d + p * 256 + lane * 4) = make_float4(dwp[p][0], dwp[p][1], dwp[p][2], dwp[p][3]);
    *reinterpret_cast<float4*>(dl_lds + wave * d + p * 256 + lane * 4) = make_float4(dlp[p][0], dlp[p][1], dlp[p][2], dlp[p][3]);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < d; j += 256) {
    const size_t off = (size_t)(blockIdx.x % copies) * copy_stride + j;
    unsafeAtomicAdd(dw_accum + off, red_lds[j] + red_lds[d + j] + red_lds[2 * d + j] + red_lds[3 * d + j]);
    if (dlam_accum) unsafeAtomicAdd(dlam_accum + off, dl_lds[j] + dl_lds[d + j] + dl_lds[2 * d + j] + dl_lds[3 * d + j]);
  }
}

}  // namespace

int k_ls_fwd(const bf16_t* res, const bf16_t* y, const bf16_t* lam, bf16_t* out, int T, int d, PathDrop D, ElemDropArg E, hipStream_t st) {
  if (T == 0) return 0;
  const int g = (int)std::min<long>(4096, ((long)T * (d / 8) + 255) / 256);
  hipLaunchKernelGGL(ls_fwd_kernel, dim3(g), dim3(256), 0, st, res, y, lam, out, (long)T, d, D, E);
  GGET_LAUNCH_CHECK();
  return 0;
}
int k_ls_rmsnorm_fwd(const bf16_t* res, const bf16_t* y, const bf16_t* lam, bf16_t* out, const bf16_t* w, bf16_t* xn, float* rstd, int T,
                     int d, float eps, PathDrop D, ElemDropArg E, hipStream_t st) {
  const int grid = (int)std::min<long>(2048, ((long)T + 3) / 4);
  if (d <= 1024) hipLaunchKernelGGL(ls_rmsnorm_fwd_kernel<2>, dim3(grid), dim3(256), 0, st, res, y, lam, out, w, xn, rstd, T, d, eps, D, E);
  else hipLaunchKernelGGL(ls_rmsnorm_fwd_kernel<4>, dim3(grid), dim3(256), 0, st, res, y, lam, out, w, xn, rstd, T, d, eps, D, E);
  GGET_LAUNCH_CHECK();
  return 0;
}
// d/8 <= 256 chunks per row (d <= 2048 is checked at create), 512 blocks; dlam: kAccumCopies replicas of align_up(d, 128) floats, or nullptr
int k_ls_bwd(const bf16_t* dy, const bf16_t* y, const bf16_t* lam, bf16_t* dsc, float* dlam, int T, int d, PathDrop D, ElemDropArg E,
             hipStream_t st) {
  if (T == 0) return 0;
  const int ls_rl = 256 / (d / 8);
  dim3 lsgrid((unsigned)std::min(512, (T + ls_rl - 1) / ls_rl));
  const size_t ls_lds_bytes = (size_t)ls_rl * d * sizeof(float);
  hipLaunchKernelGGL(ls_bwd_kernel, lsgrid, dim3(256), ls_lds_bytes, st, dy, y, lam, dsc, dlam, T, d, D, kAccumCopies,
                     align_up((uint64_t)d, 128), E);
  GGET_LAUNCH_CHECK();
  return 0;
}
int k_rmsnorm_bwd_ls(const bf16_t* dy, const bf16_t* x, const bf16_t* w, const float* rstd, const bf16_t* dres, bf16_t* dx, float* dw_accum,
                     const bf16_t* y, const bf16_t* lam, bf16_t* dsc, float* dlam_accum, int T, int d, PathDrop D, ElemDropArg E,
                     hipStream_t st) {
  if (T == 0) return 0;
  const int grid = (int)std::min<long>(4096, ((long)T + 15) / 16);
  const size_t lds = (size_t)8 * d * sizeof(float);
  const uint64_t cs = align_up((uint64_t)d, 128);
  if (!menu().ls_norm_bwd_wide && (d == 512 || d == 768 || d == 1024)) {   // (ls_norm_bwd_wide: the 16-byte-chunk form for every width)
    // 5 workgroups of 4 waves per CU in one round; every wave walks rows with a grid stride (fewer partial-sum atomics per row as well)
    const int g4 = (int)std::min<long>(1280, ((long)T + 15) / 16);
#define GGET_LS4(P) hipLaunchKernelGGL(rmsnorm_bwd_ls4_kernel<P>, dim3(g4), dim3(256), lds, st, dy, x, w, rstd, dres, dx, dw_accum, y, lam, dsc, \
                                      dlam_accum, T, kAccumCopies, cs, D, E)
    if (d == 512) GGET_LS4(2); else if (d == 768) GGET_LS4(3); else GGET_LS4(4);
#undef GGET_LS4
    GGET_LAUNCH_CHECK();
    return 0;
  }
  if (d <= 1024)
    hipLaunchKernelGGL(rmsnorm_bwd_ls_kernel<2>, dim3(grid), dim3(256), lds, st, dy, x, w, rstd, dres, dx, dw_accum, y, lam, dsc, dlam_accum, T,
                       d, kAccumCopies, cs, D, E);
  else
    hipLaunchKernelGGL(rmsnorm_bwd_ls_kernel<4>, dim3(grid), dim3(256), lds, st, dy, x, w, rstd, dres, dx, dw_accum, y, lam, dsc, dlam_accum, T,
                       d, kAccumCopies, cs, D, E);
  GGET_LAUNCH_CHECK();
  return 0;
}
