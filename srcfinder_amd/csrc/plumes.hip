// CMF-threshold plume detector (the reference's CNN-free route) and the per-plume table.
//
// Replaces srcfinder_util.py filtdet :1422-1482 with kde :1383-1387:
//   kde          g = scipy.ndimage.gaussian_filter(img, sigma=k, truncate=1) (separable correlation, axis 0 then axis 1,
//                radius int(truncate * sigma + 0.5), mode 'reflect' = d c b a | a b c d, repeated when the radius reaches
//                past the image), then img * (g - min g) / (max g - min g)                       k_gauss_cols / k_gauss_rows
//   threshold    clip((detkde - mfmin) / (mfmax - mfmin), 0, 1), ch4min = ch4mf >= mfmin, detmask = detkde > 0  k_plume_threshold
//   small ones   remove_small_objects (4-connected, size < minarea: sf_image_label4 + sf_image_filter_small_components),
//                then the removed pixels labelled 8-connected and every such component holding a pixel with
//                ch4mf >= mfminsmall put back (:1455-1463)                                       sf_plumes_restore_small
//   compaction   detcomp = imlabel(detmask); detcomp[~ch4min] = 0 without re-splitting; relabel_sequential; the
//                ~ch4min / nodata zeroing of detkde and detcomp (:1466-1477)                       sf_plumes_compact
// and the plume table the reference has no single function for: per component npix, bounding slices, sum and max of
// ch4mf with the max's first (row, col) in raster order (ime :1994-1996 is sum * ime_scale, host side).
// Everything is bit-deterministic: the blur is a fixed-order sum per output, min / max and the labelling are exact,
// the per-component sums run in a fixed order inside one workgroup per component.
#include "cmf_common.h"

namespace {

// scipy's reflect extension of a line of n samples: period 2n, a b c d d c b a
__device__ __forceinline__ int reflect_idx(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// ---- separable Gaussian, float64 ---------------------------------------------------------------------------------
// Each thread computes GC consecutive outputs of one line from an LDS tile, holding the GC + 2R inputs it needs in a
// sliding register window: (GC + 2R) / GC LDS reads and 2R + 1 FMAs per output, each in the order j = 0 .. 2R.
constexpr int PL_MAXR = 192;            // the column tile (256 + 2R rows x 32 doubles) fits 160 KiB of LDS

// axis 0 (along H): block = 32 columns x 256 output rows; 8 lane groups of 32 columns, each group GC-row chunks.
// A 32-lane half reads 32 consecutive doubles: conflict-free.
constexpr int GC_TX = 32, GC_TY = 256, GC = 8;
__global__ __launch_bounds__(256) void k_gauss_cols(const double *__restrict__ src, double *__restrict__ dst, int H, int W,
                                                     const double *__restrict__ w, int R, int absin) {
  extern __shared__ double tc[];                                 // [GC_TY + 2R][GC_TX]
  const int y0 = blockIdx.x * GC_TY, x0 = blockIdx.y * GC_TX;
  const int tx = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int x = x0 + tx, rows = GC_TY + 2 * R;
  for (int r = g; r < rows; r += 8) {
    double v = 0.0;
    if (x < W) {
      v = src[(size_t)reflect_idx(y0 - R + r, H) * W + x];
      if (absin) v = fabs(v);
    }
    tc[r * GC_TX + tx] = v;
  }
  __syncthreads();
  if (x >= W) return;
  for (int c = g; c < GC_TY / GC; c += 8) {
    const int oy = c * GC;
    if (y0 + oy >= H) break;
    double acc[GC], win[GC];
#pragma unroll
    for (int o = 0; o < GC; ++o) acc[o] = 0.0;
#pragma unroll
    for (int o = 0; o < GC - 1; ++o) win[o] = tc[(oy + o) * GC_TX + tx];
    for (int j = 0; j <= 2 * R; ++j) {
      win[GC - 1] = tc[(oy + j + GC - 1) * GC_TX + tx];
      const double wj = w[j];
#pragma unroll
      for (int o = 0; o < GC; ++o) acc[o] = fma(wj, win[o], acc[o]);
#pragma unroll
      for (int o = 0; o < GC - 1; ++o) win[o] = win[o + 1];
    }
#pragma unroll
    for (int o = 0; o < GC; ++o)
      if (y0 + oy + o < H) dst[(size_t)(y0 + oy + o) * W + x] = acc[o];
  }
}

// axis 1 (along W): one wave per row, 64 lanes x GR consecutive outputs per tile.  Lane stride GR = 5 doubles (10 dwords):
// the 32 lanes of a half hit 32 distinct bank pairs.  The block's min / max of its outputs go to partials[block] (optional).
constexpr int GR = 5, GR_TX = 64 * GR;
__global__ __launch_bounds__(256) void k_gauss_rows(const double *__restrict__ src, double *__restrict__ dst, int H, int W,
                                                     const double *__restrict__ w, int R, int absin, double *__restrict__ partials) {
  extern __shared__ double tr[];                                 // [4][GR_TX + 2R]
  __shared__ double smin[4], smax[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = blockIdx.y * 4 + wave, x0 = blockIdx.x * GR_TX;
  const int len = GR_TX + 2 * R;
  double *t = tr + wave * len;
  if (y < H) {
    const double *row = src + (size_t)y * W;
    for (int i = lane; i < len; i += 64) {
      double v = row[reflect_idx(x0 - R + i, W)];
      t[i] = absin ? fabs(v) : v;
    }
  }
  __syncthreads();
  double lo = __builtin_inf(), hi = -__builtin_inf();
  if (y < H && x0 + lane * GR < W) {
    double acc[GR], win[GR];
    const int b = lane * GR;
#pragma unroll
    for (int o = 0; o < GR; ++o) acc[o] = 0.0;
#pragma unroll
    for (int o = 0; o < GR - 1; ++o) win[o] = t[b + o];
    for (int j = 0; j <= 2 * R; ++j) {
      win[GR - 1] = t[b + j + GR - 1];
      const double wj = w[j];
#pragma unroll
      for (int o = 0; o < GR; ++o) acc[o] = fma(wj, win[o], acc[o]);
#pragma unroll
      for (int o = 0; o < GR - 1; ++o) win[o] = win[o + 1];
    }
    double *out = dst + (size_t)y * W;
#pragma unroll
    for (int o = 0; o < GR; ++o) {
      const int x = x0 + b + o;
      if (x < W) {
        out[x] = acc[o];
        lo = fmin(lo, acc[o]);
        hi = fmax(hi, acc[o]);
      }
    }
  }
  if (!partials) return;
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) { smin[wave] = lo; smax[wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partials[2 * blk] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
    partials[2 * blk + 1] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
  }
}
__global__ __launch_bounds__(1024) void k_minmax_final(const double *__restrict__ partials, int np, double *__restrict__ mm) {
  __shared__ double slo[16], shi[16];
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int i = threadIdx.x; i < np; i += 1024) { lo = fmin(lo, partials[2 * i]); hi = fmax(hi, partials[2 * i + 1]); }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) { lo = fmin(lo, slo[k]); hi = fmax(hi, shi[k]); }
    mm[0] = fmin(lo, slo[0]);
    mm[1] = fmax(hi, shi[0]);
  }
}

// ---- threshold (numpy's operation order, no contraction: the products are bit-identical to the reference's given g) -
__global__ __launch_bounds__(256) void k_plume_threshold(const double *__restrict__ ch4mf, const double *__restrict__ g,
                                                          const double *__restrict__ mm, size_t n, double mfmin, double mfmax,
                                                          int use_abs, double *__restrict__ detkde,
                                                          uint8_t *__restrict__ ch4min, uint8_t *__restrict__ detmask) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = ch4mf[i];
  double d = use_abs ? fabs(x) : x;
  if (g) d = d * ((g[i] - mm[0]) / (mm[1] - mm[0]));
  d = (d - mfmin) / (mfmax - mfmin);
  d = d < 0.0 ? 0.0 : (d > 1.0 ? 1.0 : d);                     // np.clip: NaN stays NaN
  detkde[i] = d;
  ch4min[i] = x >= mfmin;
  detmask[i] = d > 0.0;
}

// ---- restore small strong components ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_removed(const uint8_t *__restrict__ before, const uint8_t *__restrict__ after,
                                                  uint8_t *__restrict__ removed, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) removed[i] = before[i] != after[i];
}
// flags[0 .. *count] = 0 (the label space is bounded by a count that lives on the device)
__global__ __launch_bounds__(256) void k_flags_clear(uint8_t *__restrict__ flags, const int32_t *__restrict__ count) {
  const int n = *count + 1;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) flags[i] = 0;
}
__global__ __launch_bounds__(256) void k_flags_strong(const int32_t *__restrict__ labels, const double *__restrict__ ch4mf,
                                                       double thr, size_t n, uint8_t *__restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  if (l > 0 && ch4mf[i] >= thr) flags[l] = 1;                  // idempotent store: no race on the result
}
__global__ __launch_bounds__(256) void k_restore(const int32_t *__restrict__ labels, const uint8_t *__restrict__ flags, size_t n,
                                                  uint8_t *__restrict__ detmask) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  if (l > 0 && flags[l]) detmask[i] = 1;
}

// ---- compaction: surviving-label flags -> inclusive scan -> map ----------------------------------------------------
constexpr int LS_B = 1024;             // labels per scan chunk (256 threads x 4)
__global__ __launch_bounds__(256) void k_surv_clear(int32_t *__restrict__ surv, const int32_t *__restrict__ count) {
  const int n = *count + 1;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) surv[i] = 0;
}
__global__ __launch_bounds__(256) void k_surv_set(const int32_t *__restrict__ labels, const uint8_t *__restrict__ ch4min,
                                                   size_t n, int32_t *__restrict__ surv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  if (l > 0 && ch4min[i]) surv[l] = 1;
}
// inclusive scan of a 1024-entry chunk by 256 threads (4 consecutive entries each); returns the chunk total
__device__ int chunk_scan(int32_t *v, int base, int n, bool write) {
  __shared__ int wsum[4];
  int a[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = base + threadIdx.x * 4 + k;
    a[k] = i < n ? v[i] : 0;
    s += a[k];
  }
  int x = s;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(x, o, 64);
    if ((threadIdx.x & 63) >= o) x += t;
  }
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = x;
  __syncthreads();
  int off = 0;
  for (int q = 0; q < (int)(threadIdx.x >> 6); ++q) off += wsum[q];
  const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  if (write) {
    int run = off + x - s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = base + threadIdx.x * 4 + k;
      run += a[k];
      if (i < n) v[i] = run;
    }
  }
  return tot;
}
__global__ __launch_bounds__(256) void k_surv_chunksum(int32_t *__restrict__ surv, const int32_t *__restrict__ count,
                                                        int32_t *__restrict__ csum) {
  const int n = *count + 1, nc = (n + LS_B - 1) / LS_B;
  for (int c = blockIdx.x; c < nc; c += gridDim.x) {
    const int tot = chunk_scan(surv, c * LS_B, n, false);
    if (threadIdx.x == 0) csum[c] = tot;
  }
}
// exclusive scan of the chunk sums by one workgroup; *total = number of surviving labels
__global__ __launch_bounds__(1024) void k_surv_sums(int32_t *__restrict__ csum, const int32_t *__restrict__ count,
                                                     int32_t *__restrict__ total) {
  __shared__ int buf[1024];
  __shared__ int carry;
  const int nc = (*count + 1 + LS_B - 1) / LS_B;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nc; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nc ? csum[i] : 0;
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int t = threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
      __syncthreads();
      buf[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nc) csum[i] = carry + buf[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += buf[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}
// surv[l] <- number of surviving labels <= l (the new id of a surviving label l)
__global__ __launch_bounds__(256) void k_surv_apply(int32_t *__restrict__ surv, const int32_t *__restrict__ count,
                                                     const int32_t *__restrict__ csum) {
  const int n = *count + 1, nc = (n + LS_B - 1) / LS_B;
  for (int c = blockIdx.x; c < nc; c += gridDim.x) {
    chunk_scan(surv, c * LS_B, n, true);
    __syncthreads();
    const int off = csum[c];
    for (int k = threadIdx.x; k < LS_B && c * LS_B + k < n; k += 256) surv[c * LS_B + k] += off;
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_compact_apply(int32_t *__restrict__ labels, const int32_t *__restrict__ map,
                                                        const uint8_t *__restrict__ ch4min, const uint8_t *__restrict__ nodata,
                                                        double *__restrict__ detkde, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool keep = ch4min[i] && !(nodata && nodata[i]);
  const int l = labels[i];
  labels[i] = (l > 0 && keep) ? map[l] : 0;
  if (detkde && !keep) detkde[i] = 0.0;
}
__global__ void k_copy_count(const int32_t *__restrict__ src, int32_t *__restrict__ dst) { *dst = *src; }

// ---- per-component table ---------------------------------------------------------------------------------------
// irec[id][8]: npix, row start, row stop, col start, col stop, max row, max col, 0;  drec[id][2]: sum, max
__global__ void k_ptab_init(int32_t *irec, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  int32_t *r = irec + (size_t)i * 8;
  r[0] = 0; r[1] = 0x7fffffff; r[2] = 0; r[3] = 0x7fffffff; r[4] = 0; r[5] = -1; r[6] = -1; r[7] = 0;
}
__global__ __launch_bounds__(256) void k_ptab_bbox(const int32_t *__restrict__ labels, int H, int W, int ncomp,
                                                    int32_t *__restrict__ irec) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int id = labels[(size_t)y * W + x];
  if (id <= 0 || id > ncomp) return;
  int32_t *r = irec + (size_t)id * 8;
  atomicAdd(&r[0], 1);
  atomicMin(&r[1], y); atomicMax(&r[2], y + 1); atomicMin(&r[3], x); atomicMax(&r[4], x + 1);
}
// the (max, first raster index) pair of two: the larger value, on a tie the earlier index
template <typename T>
__device__ inline void keep_first_max(T &m, long long &i, T m2, long long i2) {
  if (m2 > m || (m2 == m && i2 < i)) { m = m2; i = i2; }
}
// one workgroup per component over its bounding box: thread t takes the box's pixels t, t + 256, ... in raster order,
// then a fixed tree combines the 256 partial sums and the (max, first raster index) pairs
__global__ __launch_bounds__(256) void k_ptab_stats(const int32_t *__restrict__ labels, const double *__restrict__ ch4mf,
                                                     int W, int32_t *__restrict__ irec, double *__restrict__ drec) {
  __shared__ double ssum[256], smax[256];
  __shared__ long long sidx[256];
  const int id = blockIdx.x + 1, tid = threadIdx.x;
  int32_t *r = irec + (size_t)id * 8;
  const int y0 = r[1], x0 = r[3], bw = r[4] - r[3];
  const long long bn = r[0] > 0 ? (long long)(r[2] - r[1]) * bw : 0;
  double s = 0.0, m = -__builtin_inf();
  long long mi = 0x7fffffffffffffffll;
  for (long long k = tid; k < bn; k += 256) {
    const size_t i = (size_t)(y0 + k / bw) * W + (size_t)(x0 + k % bw);
    if (labels[i] == id) {
      const double v = ch4mf[i];
      s += v;
      if (v > m) { m = v; mi = (long long)i; }                   // first in raster order: strict >
    }
  }
  ssum[tid] = s; smax[tid] = m; sidx[tid] = mi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      ssum[tid] += ssum[tid + o];
      keep_first_max(smax[tid], sidx[tid], smax[tid + o], sidx[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    drec[(size_t)id * 2] = ssum[0];
    drec[(size_t)id * 2 + 1] = smax[0];
    if (bn > 0) { r[5] = (int)(sidx[0] / W); r[6] = (int)(sidx[0] % W); }
  }
}

// the per-plume saliency: k_ptab_stats' walk and tree over the saliency map, pixels at -9999 (CNN NODATA) skipped; workgroup 0 writes
// the unused entry 0.  A component without a scored pixel: NaN, -1
__global__ __launch_bounds__(256) void k_ptab_saliency(const int32_t *__restrict__ labels, const float *__restrict__ sal, int W,
                                                        const int32_t *__restrict__ irec, float *__restrict__ smax,
                                                        int32_t *__restrict__ sidx) {
  __shared__ float sm[256];
  __shared__ long long si[256];
  const int id = blockIdx.x, tid = threadIdx.x;
  const int32_t *r = irec + (size_t)id * 8;
  const int y0 = r[1], x0 = r[3], bw = r[4] - r[3];
  const long long bn = (id > 0 && r[0] > 0) ? (long long)(r[2] - r[1]) * bw : 0;
  constexpr long long NONE = 0x7fffffffffffffffll;
  float m = -__builtin_inff();
  long long mi = NONE;
  for (long long k = tid; k < bn; k += 256) {
    const size_t i = (size_t)(y0 + k / bw) * W + (size_t)(x0 + k % bw);
    if (labels[i] == id) {
      const float v = sal[i];
      if (v != -9999.0f && v > m) { m = v; mi = (long long)i; }      // first in raster order: strict >
    }
  }
  sm[tid] = m; si[tid] = mi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) keep_first_max(sm[tid], si[tid], sm[tid + o], si[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    const bool any = si[0] != NONE;
    smax[id] = any ? sm[0] : __builtin_nanf("");
    sidx[id] = any ? (int32_t)si[0] : -1;
  }
}

dim3 grid2(int W, int H) { return dim3(sf_cdiv(W, 64), sf_cdiv(H, 4)); }
int nblk(size_t n) { return (int)((n + 255) / 256); }
// 8-connected components of an H x W mask: at most ceil(H/2) * ceil(W/2)
size_t max_components(int H, int W) { return (size_t)((H + 1) / 2) * (size_t)((W + 1) / 2); }
bool plane_ok(int H, int W) { return H >= 1 && W >= 1 && (size_t)H * W <= 0x7fffffffu; }

}  // namespace

extern "C" {

size_t sf_plumes_gauss_scratch_bytes(int H, int W) {
  if (!plane_ok(H, W)) return 0;
  return sf_align((size_t)sf_cdiv(W, GR_TX) * sf_cdiv(H, 4) * 2 * sizeof(double));
}
int sf_plumes_gauss_pass(const double *src, double *dst, int H, int W, int axis, const double *weights, int radius, int absin,
                         double *minmax, void *scratch, void *stream) {
  if (!src || !dst || !weights || src == dst || !plane_ok(H, W) || (axis != 0 && axis != 1) || radius < 0 ||
      radius > PL_MAXR || (minmax && (axis != 1 || !scratch))) {
    sf_set_error("sf_plumes_gauss_pass: bad argument (radius must lie in 0..%d; minmax only with axis 1 and scratch)", PL_MAXR);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  if (axis == 0) {
    const size_t lds = (size_t)(GC_TY + 2 * radius) * GC_TX * sizeof(double);
    if (int rc = sf_lds_attr(reinterpret_cast<const void *>(k_gauss_cols), lds)) return rc;
    hipLaunchKernelGGL(k_gauss_cols, dim3(sf_cdiv(H, GC_TY), sf_cdiv(W, GC_TX)), dim3(256), lds, st, src, dst, H, W, weights,
                       radius, absin);
    SF_LAUNCH_CHECK("k_gauss_cols");
    return 0;
  }
  const size_t lds = (size_t)4 * (GR_TX + 2 * radius) * sizeof(double);
  if (int rc = sf_lds_attr(reinterpret_cast<const void *>(k_gauss_rows), lds)) return rc;
  const dim3 grid(sf_cdiv(W, GR_TX), sf_cdiv(H, 4));
  double *partials = minmax ? reinterpret_cast<double *>(scratch) : nullptr;
  hipLaunchKernelGGL(k_gauss_rows, grid, dim3(256), lds, st, src, dst, H, W, weights, radius, absin, partials);
  SF_LAUNCH_CHECK("k_gauss_rows");
  if (minmax) {
    hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(1024), 0, st, partials, (int)(grid.x * grid.y), minmax);
    SF_LAUNCH_CHECK("k_minmax_final");
  }
  return 0;
}

int sf_plumes_threshold(const double *ch4mf, const double *g, const double *minmax, int H, int W, double mfmin, double mfmax,
                        int use_abs, double *detkde, uint8_t *ch4min, uint8_t *detmask, void *stream) {
  if (!ch4mf || !detkde || !ch4min || !detmask || (g && !minmax) || !plane_ok(H, W)) {
    sf_set_error("sf_plumes_threshold: bad argument");
    return -1;
  }
  const size_t n = (size_t)H * W;
  hipLaunchKernelGGL(k_plume_threshold, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, ch4mf, g, minmax, n, mfmin, mfmax,
                     use_abs, detkde, ch4min, detmask);
  SF_LAUNCH_CHECK("k_plume_threshold");
  return 0;
}

size_t sf_plumes_restore_scratch_bytes(int H, int W) {
  if (!plane_ok(H, W)) return 0;
  const size_t n = (size_t)H * W;
  return sf_align(n) + sf_align(n * sizeof(int32_t)) + sf_align(sizeof(int32_t)) + sf_align(max_components(H, W) + 1) +
         sf_image_label8_scratch_bytes(H, W);
}
int sf_plumes_restore_small(const uint8_t *detsmall, uint8_t *detmask, const double *ch4mf, double mfminsmall, int H, int W,
                            void *scratch, void *stream) {
  if (!detsmall || !detmask || !ch4mf || !scratch || !plane_ok(H, W)) {
    sf_set_error("sf_plumes_restore_small: bad argument");
    return -1;
  }
  const size_t n = (size_t)H * W;
  char *p = reinterpret_cast<char *>(scratch);
  uint8_t *removed = reinterpret_cast<uint8_t *>(p); p += sf_align(n);
  int32_t *lab = reinterpret_cast<int32_t *>(p); p += sf_align(n * sizeof(int32_t));
  int32_t *cnt = reinterpret_cast<int32_t *>(p); p += sf_align(sizeof(int32_t));
  uint8_t *flags = reinterpret_cast<uint8_t *>(p); p += sf_align(max_components(H, W) + 1);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_removed, dim3(nblk(n)), dim3(256), 0, st, detsmall, detmask, removed, n);
  SF_LAUNCH_CHECK("k_removed");
  if (int rc = sf_image_label8(removed, H, W, lab, nullptr, 0, cnt, p, stream)) return rc;
  hipLaunchKernelGGL(k_flags_clear, dim3(1024), dim3(256), 0, st, flags, cnt);
  SF_LAUNCH_CHECK("k_flags_clear");
  hipLaunchKernelGGL(k_flags_strong, dim3(nblk(n)), dim3(256), 0, st, lab, ch4mf, mfminsmall, n, flags);
  SF_LAUNCH_CHECK("k_flags_strong");
  hipLaunchKernelGGL(k_restore, dim3(nblk(n)), dim3(256), 0, st, lab, flags, n, detmask);
  SF_LAUNCH_CHECK("k_restore");
  return 0;
}

size_t sf_plumes_compact_scratch_bytes(int H, int W) {
  if (!plane_ok(H, W)) return 0;
  const size_t nl = max_components(H, W) + 1;
  return sf_align(nl * sizeof(int32_t)) + sf_align(((nl + LS_B - 1) / LS_B) * sizeof(int32_t)) + sf_align(sizeof(int32_t));
}
int sf_plumes_compact(int32_t *labels, int32_t *ncomp_dev, const uint8_t *ch4min, const uint8_t *nodata, double *detkde, int H,
                      int W, void *scratch, void *stream) {
  if (!labels || !ncomp_dev || !ch4min || !scratch || !plane_ok(H, W)) {
    sf_set_error("sf_plumes_compact: bad argument");
    return -1;
  }
  const size_t n = (size_t)H * W, nl = max_components(H, W) + 1;
  char *p = reinterpret_cast<char *>(scratch);
  int32_t *surv = reinterpret_cast<int32_t *>(p); p += sf_align(nl * sizeof(int32_t));
  int32_t *csum = reinterpret_cast<int32_t *>(p); p += sf_align(((nl + LS_B - 1) / LS_B) * sizeof(int32_t));
  int32_t *total = reinterpret_cast<int32_t *>(p);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_surv_clear, dim3(1024), dim3(256), 0, st, surv, ncomp_dev);
  SF_LAUNCH_CHECK("k_surv_clear");
  hipLaunchKernelGGL(k_surv_set, dim3(nblk(n)), dim3(256), 0, st, labels, ch4min, n, surv);
  SF_LAUNCH_CHECK("k_surv_set");
  hipLaunchKernelGGL(k_surv_chunksum, dim3(1024), dim3(256), 0, st, surv, ncomp_dev, csum);
  SF_LAUNCH_CHECK("k_surv_chunksum");
  hipLaunchKernelGGL(k_surv_sums, dim3(1), dim3(1024), 0, st, csum, ncomp_dev, total);
  SF_LAUNCH_CHECK("k_surv_sums");
  hipLaunchKernelGGL(k_surv_apply, dim3(1024), dim3(256), 0, st, surv, ncomp_dev, csum);
  SF_LAUNCH_CHECK("k_surv_apply");
  hipLaunchKernelGGL(k_compact_apply, dim3(nblk(n)), dim3(256), 0, st, labels, surv, ch4min, nodata, detkde, n);
  SF_LAUNCH_CHECK("k_compact_apply");
  hipLaunchKernelGGL(k_copy_count, dim3(1), dim3(1), 0, st, total, ncomp_dev);
  SF_LAUNCH_CHECK("k_copy_count");
  return 0;
}

int sf_plumes_stats(const int32_t *labels, const double *ch4mf, int H, int W, int ncomp, int32_t *irec, double *drec,
                    void *stream) {
  if (!labels || !ch4mf || !irec || !drec || !plane_ok(H, W) || ncomp < 0) {
    sf_set_error("sf_plumes_stats: bad argument");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ptab_init, dim3(sf_cdiv(ncomp + 1, 256)), dim3(256), 0, st, irec, ncomp);
  SF_LAUNCH_CHECK("k_ptab_init");
  if (ncomp == 0) return 0;
  hipLaunchKernelGGL(k_ptab_bbox, grid2(W, H), dim3(256), 0, st, labels, H, W, ncomp, irec);
  SF_LAUNCH_CHECK("k_ptab_bbox");
  hipLaunchKernelGGL(k_ptab_stats, dim3(ncomp), dim3(256), 0, st, labels, ch4mf, W, irec, drec);
  SF_LAUNCH_CHECK("k_ptab_stats");
  return 0;
}

int sf_plumes_saliency(const int32_t *labels, const float *sal, int H, int W, int ncomp, const int32_t *irec, float *smax,
                       int32_t *sidx, void *stream) {
  if (!labels || !sal || !irec || !smax || !sidx || !plane_ok(H, W) || ncomp < 0) {
    sf_set_error("sf_plumes_saliency: bad argument");
    return -1;
  }
  hipLaunchKernelGGL(k_ptab_saliency, dim3(ncomp + 1), dim3(256), 0, (hipStream_t)stream, labels, sal, W, irec, smax, sidx);
  SF_LAUNCH_CHECK("k_ptab_saliency");
  return 0;
}

}  // extern "C"
