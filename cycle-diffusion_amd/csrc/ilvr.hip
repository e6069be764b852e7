// ILVR conditioning (Choi et al., ICCV 2021): after a decode step x',
//   x <- x' + phi_N(y' - x'),   y' = qa*y + qb*n,   phi_N(X) = U D X D^T U^T per channel image,
// D [r, R] the antialiased cubic down-by-N, U [R, r] the cubic up-by-N (r = R / N), both as tap lists (kernels.h LowpassTaps).
// fp32 throughout, contraction off. Two launches:
//   k_ilvr_down    one workgroup per (output row i, channel, sample): the band of P_D image rows under row i of D is formed
//                  from x', y and the draw on the fly, staged through LDS a chunk of rows at a time (16-byte global loads), and
//                  summed down each column, V[i, :] = sum_t D[i, t] d[first_i + t, :]; then T[i, k] = sum_t D[k, t] V[i, first_k + t].
//                  d = y' - x' never reaches HBM; bands of neighbouring rows overlap about 4 x and are re-formed.
//   k_ilvr_up_add  one workgroup per (4 output rows, channel, sample): W[X, :] = sum_t U[X, t] T[first_X + t, :] into LDS,
//                  out[X, Y] = x'[X, Y] + sum_t W[X, first_Y + t] U[Y, t]; writes x and the next forward's 16-bit input.
// Every sum runs over its taps in ascending order with a compensation term (Kahan): a row of D has 4 N + 2 taps (130 at
// N = 32), and a constant image has to come back to a few units in the last place. No atomics; a sample's result depends on
// nothing but its own tensors.
#include "common.h"
#include "gauss.h"
#include "kernels.h"

#include <cmath>

namespace cd {

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kColsPerThread = kIlvrMaxR / kThreads;  // column accumulators of a thread of k_ilvr_down
constexpr int kBandFloats = 4096;                     // LDS band chunk: max(1, kBandFloats / R) image rows
constexpr int kUpRows = 4;                            // output rows per workgroup of k_ilvr_up_add

__device__ inline void kahan_add(float& acc, float& cmp, float v) {
  float yk = v - cmp;
  float t = acc + yk;
  cmp = (t - acc) - yk;
  acc = t;
}

// d = (qa*y + qb*n) - x' of element `at` of the running image (`yat` of the reference)
__device__ inline float form_d(const IlvrArgs& a, float qa, float qb, int64_t at, int64_t yat) {
  float yp = qa * a.y[yat];
  if (qb != 0.f) {
    float a1 = qb * draw(a.gauss, at);
    yp = yp + a1;
  }
  return a.xp ? yp - a.xp[at] : yp;
}

__device__ inline float4 form_d4(const IlvrArgs& a, float qa, float qb, int64_t at, int64_t yat) {
  const float4 yv = *(const float4*)(a.y + yat);
  float4 yp = make_float4(qa * yv.x, qa * yv.y, qa * yv.z, qa * yv.w);
  if (qb != 0.f) {
    float4 nz;
    if (a.gauss.noise) nz = *(const float4*)(a.gauss.noise + at);
    else nz = make_float4(draw(a.gauss, at), draw(a.gauss, at + 1), draw(a.gauss, at + 2), draw(a.gauss, at + 3));
    float4 a1 = make_float4(qb * nz.x, qb * nz.y, qb * nz.z, qb * nz.w);
    yp = make_float4(yp.x + a1.x, yp.y + a1.y, yp.z + a1.z, yp.w + a1.w);
  }
  if (!a.xp) return yp;
  const float4 xv = *(const float4*)(a.xp + at);
  return make_float4(yp.x - xv.x, yp.y - xv.y, yp.z - xv.z, yp.w - xv.w);
}

__global__ void __launch_bounds__(kThreads) k_ilvr_down(IlvrArgs a) {
  extern __shared__ float smem[];
  const int R = a.R, r = a.D.n_out, P = a.D.P;
  const int i = blockIdx.x, c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int p4 = (P + 3) & ~3, r4 = (R + 3) & ~3;
  float* sW = smem;        // row i of D, P taps
  float* sV = sW + p4;     // V[i, :], R columns
  float* sB = sV + r4;     // band chunk [rows][R]
  const int chunk = kBandFloats / R > 0 ? kBandFloats / R : 1;
  float qa = 1.f, qb = 0.f;
  if (a.qtab) { const float2 q = a.qtab[a.qrow]; qa = q.x; qb = q.y; }
  for (int t = tid; t < P; t += kThreads) sW[t] = a.D.w[(int64_t)t * r + i];
  const int f = a.D.first[i];
  const int64_t plane = ((int64_t)b * a.C + c) * R * R, yplane = ((int64_t)(b % a.y_bmod) * a.C + c) * R * R;
  float acc[kColsPerThread], cmp[kColsPerThread];
#pragma unroll
  for (int q = 0; q < kColsPerThread; ++q) acc[q] = cmp[q] = 0.f;
  for (int t0 = 0; t0 < P; t0 += chunk) {
    const int rows = P - t0 < chunk ? P - t0 : chunk;
    const int64_t off = (int64_t)(f + t0) * R;  // the band's rows are contiguous in the image
    __syncthreads();                            // the previous chunk is consumed (first pass: sW is written)
    if (a.vec4) {
      for (int e = tid * 4; e < rows * R; e += kThreads * 4)
        *(float4*)(sB + e) = form_d4(a, qa, qb, plane + off + e, yplane + off + e);
    } else {
      for (int e = tid; e < rows * R; e += kThreads) sB[e] = form_d(a, qa, qb, plane + off + e, yplane + off + e);
    }
    __syncthreads();
    for (int tt = 0; tt < rows; ++tt) {
      const float w = sW[t0 + tt];
#pragma unroll
      for (int q = 0; q < kColsPerThread; ++q) {
        const int x = tid + q * kThreads;
        if (x < R) kahan_add(acc[q], cmp[q], w * sB[tt * R + x]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kColsPerThread; ++q) {
    const int x = tid + q * kThreads;
    if (x < R) sV[x] = acc[q];
  }
  __syncthreads();
  float* Trow = a.T + (((int64_t)b * a.C + c) * r + i) * r;
  for (int k = tid; k < r; k += kThreads) {
    const int fk = a.D.first[k];
    float s = 0.f, cs = 0.f;
    for (int t = 0; t < P; ++t) kahan_add(s, cs, a.D.w[(int64_t)t * r + k] * sV[fk + t]);
    Trow[k] = s;
  }
}

__device__ inline void store_xin(const XinOut& o, int B, int HW, int cpad_c, int b, int p, float v) {
  bf16_t h = f2bf(v);
  size_t at = ((size_t)b * HW + p) * o.cpad + cpad_c;
  o.xin[at] = h;
  if (o.dup) o.xin[at + (size_t)B * HW * o.cpad] = h;
}

__global__ void __launch_bounds__(kThreads) k_ilvr_up_add(IlvrArgs a) {
  extern __shared__ float sWr[];  // W[X0 .. X0 + kUpRows - 1, :], r columns each
  const int R = a.R, r = a.U.n_in, P = a.U.P;
  const int X0 = blockIdx.x * kUpRows, c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const float* Tp = a.T + ((int64_t)b * a.C + c) * r * r;
  for (int idx = tid; idx < kUpRows * r; idx += kThreads) {
    const int xr = idx / r, k = idx - xr * r, X = X0 + xr;
    float s = 0.f, cs = 0.f;
    if (X < R) {
      const int fx = a.U.first[X];
      for (int t = 0; t < P; ++t) kahan_add(s, cs, a.U.w[(int64_t)t * R + X] * Tp[(fx + t) * r + k]);
    }
    sWr[idx] = s;
  }
  __syncthreads();
  const int64_t plane = ((int64_t)b * a.C + c) * R * R;
  if (a.vec4) {
    const int qr = R / 4;
    for (int q = tid; q < kUpRows * qr; q += kThreads) {
      const int xr = q / qr, Y = (q - xr * qr) * 4, X = X0 + xr;
      if (X >= R) continue;
      const int4 fy = *(const int4*)(a.U.first + Y);
      const float* wrow = sWr + xr * r;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f), cs = s;
      for (int t = 0; t < P; ++t) {
        const float4 w = *(const float4*)(a.U.w + (int64_t)t * R + Y);
        kahan_add(s.x, cs.x, wrow[fy.x + t] * w.x);
        kahan_add(s.y, cs.y, wrow[fy.y + t] * w.y);
        kahan_add(s.z, cs.z, wrow[fy.z + t] * w.z);
        kahan_add(s.w, cs.w, wrow[fy.w + t] * w.w);
      }
      const int64_t at = plane + (int64_t)X * R + Y;
      if (a.xp) {
        const float4 xv = *(const float4*)(a.xp + at);
        s = make_float4(xv.x + s.x, xv.y + s.y, xv.z + s.z, xv.w + s.w);
      }
      *(float4*)(a.out + at) = s;
      if (a.xin.xin) {
        const int p = X * R + Y;
        store_xin(a.xin, a.B, R * R, c, b, p, s.x);
        store_xin(a.xin, a.B, R * R, c, b, p + 1, s.y);
        store_xin(a.xin, a.B, R * R, c, b, p + 2, s.z);
        store_xin(a.xin, a.B, R * R, c, b, p + 3, s.w);
      }
    }
  } else {
    for (int q = tid; q < kUpRows * R; q += kThreads) {
      const int xr = q / R, Y = q - xr * R, X = X0 + xr;
      if (X >= R) continue;
      const int fy = a.U.first[Y];
      float s = 0.f, cs = 0.f;
      for (int t = 0; t < P; ++t) kahan_add(s, cs, sWr[xr * r + fy + t] * a.U.w[(int64_t)t * R + Y]);
      const int64_t at = plane + (int64_t)X * R + Y;
      if (a.xp) s = a.xp[at] + s;
      a.out[at] = s;
      if (a.xin.xin) store_xin(a.xin, a.B, R * R, c, b, X * R + Y, s);
    }
  }
}

double keys_cubic(double x) {
  const double A = -0.5;
  x = std::fabs(x);
  if (x <= 1.0) return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
  if (x < 2.0) return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A;
  return 0.0;
}

}  // namespace

void build_lowpass_taps(int n_in, int n_out, std::vector<float>& w, std::vector<int>& first, int& P) {
  const double s = (double)n_out / n_in, width = s < 1.0 ? 4.0 / s : 4.0;
  const int taps = (int)std::ceil(width) + 2;
  P = taps < n_in ? taps : n_in;
  w.assign((size_t)P * n_out, 0.f);
  first.assign(n_out, 0);
  std::vector<double> raw(taps), row(n_in);
  for (int i = 0; i < n_out; ++i) {
    const double u = (i + 0.5) / s - 0.5;
    const int j0 = (int)std::floor(u - width / 2.0) + 1;
    double sum = 0.0;
    for (int t = 0; t < taps; ++t) {
      raw[t] = s < 1.0 ? s * keys_cubic(s * (u - (j0 + t))) : keys_cubic(u - (j0 + t));
      sum += raw[t];
    }
    std::fill(row.begin(), row.end(), 0.0);
    for (int t = 0; t < taps; ++t) {
      int j = j0 + t;
      if (j < 0) j = -j - 1;
      else if (j >= n_in) j = 2 * n_in - 1 - j;
      CD_CHECK(j >= 0 && j < n_in, "low-pass taps: one reflection does not suffice for a %d -> %d resize", n_in, n_out);
      row[j] += raw[t] / sum;
    }
    const int f = j0 < 0 ? 0 : (j0 > n_in - P ? n_in - P : j0);
    first[i] = f;
    for (int j = 0; j < n_in; ++j)
      CD_CHECK(row[j] == 0.0 || (j >= f && j < f + P), "low-pass taps: a weight of row %d lies outside its window", i);
    for (int t = 0; t < P; ++t) w[(size_t)t * n_out + i] = (float)row[f + t];
  }
}

static void check_ilvr(const IlvrArgs& a) {
  const int r = a.D.n_out;
  CD_CHECK(a.R > 0 && a.R <= kIlvrMaxR, "the low-pass kernels take images of at most %d pixels a side, got %d", kIlvrMaxR, a.R);
  CD_CHECK(a.D.n_in == a.R && a.U.n_out == a.R && a.U.n_in == r && a.D.P <= a.R && a.U.P <= r, "low-pass tap tables do not fit");
  CD_CHECK(a.B > 0 && a.B <= 65535 && a.C > 0 && a.C <= 65535 && a.y_bmod > 0, "bad low-pass batch");
}

void launch_ilvr_down(hipStream_t st, const IlvrArgs& a) {
  check_ilvr(a);
  const int R = a.R, chunk = kBandFloats / R > 0 ? kBandFloats / R : 1;
  const size_t lds = (size_t)(((a.D.P + 3) & ~3) + ((R + 3) & ~3) + chunk * R) * sizeof(float);
  hipLaunchKernelGGL(k_ilvr_down, dim3(a.D.n_out, a.C, a.B), dim3(kThreads), lds, st, a);
}

void launch_ilvr_up_add(hipStream_t st, const IlvrArgs& a) {
  check_ilvr(a);
  const size_t lds = (size_t)kUpRows * a.U.n_in * sizeof(float);
  hipLaunchKernelGGL(k_ilvr_up_add, dim3((a.R + kUpRows - 1) / kUpRows, a.C, a.B), dim3(kThreads), lds, st, a);
}

}  // namespace cd
