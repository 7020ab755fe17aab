// mogan_attn_sheet.hip -- the device side of the attention sheets of DESIGN.md section 9p: what miscc/vis.build_super_images2 does on
// the host per word (threshold, bilinear upscaling, Gaussian smoothing, min-max normalisation, 8-bit quantisation, Pillow's paste
// over the image) in one launch.  attngan/attnsheet.py holds the definition and the numpy oracle (conf_numpy, sheet_numpy).  The
// upscaling and the smoothing are one table M (vis x att) the host builds; the kernel never sees sigma.  Everything after the fp32
// loads is fp64.
//
// attn_conf_kernel: one workgroup per (sample, word); thread t adds a [a > 4 / len] over the elements t, t + NT, ... in that order,
// the NT partials are added in LDS in a fixed binary tree.  No atomics.
//
// attn_sheet_kernel: one workgroup of 256 threads per pick, so a pick's arithmetic does not depend on where in the list it stands,
// and lo and hi never leave the workgroup.  The thresholded map A goes to LDS once as fp32.  S = M A M^T is formed in strips of
// R = 32 output rows:
//     U[r][k] = sum_j M[r0 + r][j] A[j][k]      j ascending, one fma per term      (R x att, LDS)
//     S[r][c] = sum_k U[r][k] M[c][k]           k ascending, one fma per term      (registers: 8 rows x 4 columns per thread)
// and the product is walked twice in this one order: the first walk takes min and max, the second quantises, blends and writes --
// the (vis x vis) fp64 map never exists in memory.  A wave owns 8 rows of the strip, a lane the columns lane, lane + 64, ...: the
// rows' operands are broadcast reads, the columns' are conflict-free.  M's rows of the strip and, for the second product, chunks of
// 16 columns of M transposed are staged in one LDS buffer.  Lanes past the last column repeat it and rows past the last row are
// zeros: no uninitialised word is read, and neither is stored.  A map's odd row count is padded with one zero term, which adds
// +0.0 to a sum that is never -0.0.
//
// With the identity table every sum has one non-zero term 1.0 * a: S is A exactly.  A map where nothing passes the threshold is
// exact zeros, lo == hi, flag 1.  A pick outside the batch or at or past its caption's length is answered before anything is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

namespace {

constexpr int NT = 256;
constexpr int ATT_MIN = 2, ATT_MAX = 128, VIS_MAX = 256, T_MAX = 32;
constexpr int R = 32;                          // output rows per strip: 8 per wave
constexpr int RW = 8;                          // rows a wave owns
constexpr int CW = 4;                          // columns a lane owns in the second product (vis <= 256)
constexpr int KW = 2;                          // columns a lane owns in the first (att <= 128)
constexpr int KC = 16;                         // columns of M per staged chunk
constexpr int VP = VIS_MAX + 1;                // row pitch of the transposed chunk: the staging stores spread over the banks
constexpr long long I31 = 2147483647LL;

__host__ __device__ inline int even_up(int n) { return (n + 1) & ~1; }
// LDS, in bytes: A as fp32 with one zero row behind an odd att | U [att][R] fp64 | the staging buffer, M's strip or a chunk of M^T
__host__ __device__ inline size_t a_bytes(int att) { return (((size_t)even_up(att) * att * 4) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t u_bytes(int att) { return (size_t)att * R * 8; }
__host__ __device__ inline size_t s_bytes(int att) {
    const size_t strip = (size_t)R * even_up(att) * 8, chunk = (size_t)KC * VP * 8;
    return strip > chunk ? strip : chunk;
}

__global__ __launch_bounds__(NT) void attn_conf_kernel(const float* __restrict__ attn, const int* __restrict__ cap_lens, int T, int att,
                                                       double* __restrict__ conf) {
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const size_t bt = blockIdx.x;
    const int b = (int)(bt / T), t = (int)(bt % T);
    const int len = cap_lens[b];
    if (t >= len) {                                                 // uniform over the workgroup (len < 1 too)
        if (tid == 0) conf[bt] = 0.0;
        return;
    }
    const float t4 = 2.f * (float)(2.0 / (double)len);
    const float* a = attn + bt * (size_t)att * att;
    const int n = att * att;
    double acc = 0.0;
    for (int i = tid; i < n; i += NT) {
        const float v = a[i];
        acc += (double)v * (v > t4 ? 1.0 : 0.0);                    // a [a > t] as the oracle writes it: a NaN stays one
    }
    red[tid] = acc;
    __syncthreads();
    for (int off = NT / 2; off >= 1; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) conf[bt] = red[0];
}

__device__ inline unsigned image_byte(float x) {
    float f = (x + 1.f) / 2.f * 255.f;                              // the fp32 roundings of the host's ((x + 1) / 2 * 255)
    f = f >= 0.f ? (f <= 255.f ? f : 255.f) : 0.f;                  // a NaN becomes 0
    return (unsigned)(int)f;
}

__device__ inline unsigned char paste(unsigned image, unsigned q, unsigned alpha) {       // Pillow's BLEND8 through a constant mask
    const unsigned t = image * (255u - alpha) + q * alpha + 128u;
    return (unsigned char)(((t >> 8) + t) >> 8);
}

__global__ __launch_bounds__(NT) void attn_sheet_kernel(const float* __restrict__ attn, const int* __restrict__ cap_lens,
                                                        const float* __restrict__ img, const double* __restrict__ table,
                                                        const int* __restrict__ pick, int B, int T, int att, int vis, int alpha,
                                                        unsigned char* __restrict__ sheet, double* __restrict__ stats,
                                                        int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ double red_lo[NT], red_hi[NT];
    __shared__ int red_bad[NT];
    float* A_s = reinterpret_cast<float*>(lds);                                       // [even_up(att)][att]
    double* U_s = reinterpret_cast<double*>(lds + a_bytes(att));                      // [att][R]
    double* St = reinterpret_cast<double*>(lds + a_bytes(att) + u_bytes(att));        // [R][ap] or [KC][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t p = blockIdx.x;
    const int b = pick[2 * p], t = pick[2 * p + 1];
    unsigned char* out = sheet + p * (size_t)vis * vis * 3;
    const int n_out = vis * vis * 3;
    int len = 0;
    bool ok = b >= 0 && b < B && t >= 0 && t < T;
    if (ok) { len = cap_lens[b]; ok = t < len; }
    if (!ok) {                                                      // uniform over the workgroup: nobody reaches a barrier
        for (int i = tid; i < n_out; i += NT) out[i] = 0;
        if (tid == 0) { stats[2 * p] = 0.0; stats[2 * p + 1] = 0.0; flags[p] = 3; }
        return;
    }
    const int ap = even_up(att);
    const float t2 = (float)(2.0 / (double)len);
    const float* a = attn + ((size_t)b * T + t) * (size_t)att * att;
    for (int i = tid; i < ap * att; i += NT) {
        const float v = i < att * att ? a[i] : 0.f;
        A_s[i] = v * (v > t2 ? 1.f : 0.f);                          // a [a > t] as the oracle writes it: a NaN stays one
    }
    int kcol[KW], ccol[CW];                                         // lanes past the last column repeat it; nothing of theirs is kept
#pragma unroll
    for (int i = 0; i < KW; ++i) kcol[i] = min(lane + 64 * i, att - 1);
#pragma unroll
    for (int i = 0; i < CW; ++i) ccol[i] = min(lane + 64 * i, vis - 1);
    const float* im = img + (size_t)b * 3 * vis * vis;
    double lo = 0.0, hi = 0.0, scale = 0.0;
    int flag = 0;
    for (int pass = 0; pass < 2; ++pass) {
        double my_lo = __longlong_as_double(0x7FF0000000000000LL), my_hi = -my_lo;
        int my_bad = 0;
        for (int r0 = 0; r0 < vis; r0 += R) {
            __syncthreads();                                        // A_s is complete; the strip before this one is consumed
            if (flag == 0) {
                // M's rows r0 .. r0 + R - 1, zeros past the last row and in the pad column
                for (int i = tid; i < R * ap; i += NT) {
                    const int r = i / ap, j = i - r * ap;
                    St[i] = (r0 + r < vis && j < att) ? table[(size_t)(r0 + r) * att + j] : 0.0;
                }
                __syncthreads();
                {
                    double acc[RW][KW];
#pragma unroll
                    for (int r = 0; r < RW; ++r)
#pragma unroll
                        for (int i = 0; i < KW; ++i) acc[r][i] = 0.0;
                    const double* ms = St + (size_t)(wave * RW) * ap;
                    for (int j = 0; j < ap; j += 2) {
                        double a0[KW], a1[KW];
#pragma unroll
                        for (int i = 0; i < KW; ++i) {
                            a0[i] = (double)A_s[j * att + kcol[i]];
                            a1[i] = (double)A_s[(j + 1) * att + kcol[i]];
                        }
#pragma unroll
                        for (int r = 0; r < RW; ++r) {
                            const double2 m = *reinterpret_cast<const double2*>(ms + r * ap + j);
#pragma unroll
                            for (int i = 0; i < KW; ++i) {
                                acc[r][i] = fma(m.x, a0[i], acc[r][i]);
                                acc[r][i] = fma(m.y, a1[i], acc[r][i]);
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < KW; ++i) {
                        const int k = lane + 64 * i;
                        if (k < att) {
#pragma unroll
                            for (int r = 0; r < RW; ++r) U_s[k * R + wave * RW + r] = acc[r][i];
                        }
                    }
                }
            }
            double s[RW][CW];
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int i = 0; i < CW; ++i) s[r][i] = 0.0;
            if (flag == 0) {
                for (int k0 = 0; k0 < att; k0 += KC) {
                    const int kc = min(KC, att - k0);
                    __syncthreads();                                // U_s is complete; the chunk (or the strip) before is consumed
                    for (int i = tid; i < vis * KC; i += NT) {
                        const int c = i / KC, kk = i - c * KC;
                        St[kk * VP + c] = kk < kc ? table[(size_t)c * att + k0 + kk] : 0.0;
                    }
                    __syncthreads();
                    for (int kk = 0; kk < kc; ++kk) {
                        double m[CW];
#pragma unroll
                        for (int i = 0; i < CW; ++i) m[i] = St[kk * VP + ccol[i]];
                        const double* u = U_s + (k0 + kk) * R + wave * RW;
#pragma unroll
                        for (int r = 0; r < RW; r += 2) {
                            const double2 uv = *reinterpret_cast<const double2*>(u + r);
#pragma unroll
                            for (int i = 0; i < CW; ++i) {
                                s[r][i] = fma(uv.x, m[i], s[r][i]);
                                s[r + 1][i] = fma(uv.y, m[i], s[r + 1][i]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const int y = r0 + wave * RW + r;
#pragma unroll
                for (int i = 0; i < CW; ++i) {
                    const int x = lane + 64 * i;
                    if (y < vis && x < vis) {
                        const double v = s[r][i];
                        if (pass == 0) {
                            my_bad |= !(fabs(v) <= 1.7976931348623157e308);
                            my_lo = fmin(my_lo, v);
                            my_hi = fmax(my_hi, v);
                        } else {
                            unsigned q = 0;
                            if (flag == 0) q = (unsigned)(int)((v - lo) / scale * 255.0);
                            const size_t px = (size_t)y * vis + x;
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                out[px * 3 + c] = paste(image_byte(im[(size_t)c * vis * vis + px]), q, (unsigned)alpha);
                        }
                    }
                }
            }
        }
        if (pass == 0) {
            red_lo[tid] = my_lo; red_hi[tid] = my_hi; red_bad[tid] = my_bad;
            __syncthreads();
            for (int off = NT / 2; off >= 1; off >>= 1) {
                if (tid < off) {
                    red_lo[tid] = fmin(red_lo[tid], red_lo[tid + off]);
                    red_hi[tid] = fmax(red_hi[tid], red_hi[tid + off]);
                    red_bad[tid] |= red_bad[tid + off];
                }
                __syncthreads();
            }
            lo = red_lo[0]; hi = red_hi[0];
            flag = red_bad[0] ? 2 : (hi == lo ? 1 : 0);
            if (flag == 2) { lo = 0.0; hi = 0.0; }
            scale = hi - lo;
            if (tid == 0) { stats[2 * p] = lo; stats[2 * p + 1] = hi; flags[p] = flag; }
        }
    }
}

}  // namespace

extern "C" {

int mogan_attn_conf_f64(const float* attn, const int* cap_lens, int B, int T, int att, double* conf, hipStream_t stream) {
    if (!attn || !cap_lens || !conf || B < 1 || T < 1 || T > T_MAX || att < ATT_MIN || att > ATT_MAX) return MOGAN_ERR_SHAPE;
    if (B > I31 / ((long long)T * att * att)) return MOGAN_ERR_SHAPE;                             // B T att att <= 2^31 - 1
    hipLaunchKernelGGL(attn_conf_kernel, dim3((unsigned)(B * T)), dim3(NT), 0, stream, attn, cap_lens, T, att, conf);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_attn_sheet_f64(const float* attn, const int* cap_lens, const float* img, const double* table, const int* pick, int P, int B,
                         int T, int att, int vis, int alpha, unsigned char* sheet, double* stats, int* flags, hipStream_t stream) {
    if (!attn || !cap_lens || !img || !table || !pick || !sheet || !stats || !flags) return MOGAN_ERR_SHAPE;
    if (P < 1 || B < 1 || T < 1 || T > T_MAX || att < ATT_MIN || att > ATT_MAX || vis < att || vis > VIS_MAX || vis % att != 0
        || alpha < 0 || alpha > 255)
        return MOGAN_ERR_SHAPE;
    if (B > I31 / ((long long)T * att * att) || B > I31 / (3LL * vis * vis) || P > I31 / (3LL * vis * vis)) return MOGAN_ERR_SHAPE;
    if ((((uintptr_t)table | (uintptr_t)stats) & 7) != 0) return MOGAN_ERR_SHAPE;
    const size_t lds = a_bytes(att) + u_bytes(att) + s_bytes(att);                                // at most 131 328 bytes
    static bool attr = false;                                                                     // dynamic LDS beyond 64 KiB
    if (!attr) {
        if (hipFuncSetAttribute((const void*)attn_sheet_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024) != hipSuccess) {
            (void)hipGetLastError();
            return MOGAN_ERR_LAUNCH;
        }
        attr = true;
    }
    hipLaunchKernelGGL(attn_sheet_kernel, dim3((unsigned)P), dim3(NT), lds, stream, attn, cap_lens, img, table, pick, B, T, att, vis,
                       alpha, sheet, stats, flags);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

}  // extern "C"
