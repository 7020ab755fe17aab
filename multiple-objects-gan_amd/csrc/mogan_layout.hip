// mogan_layout.hip -- the device side of the layout-shift score of DESIGN.md section 9n: what changes between an image generated
// under the data's layout (a) and the image generated from the same noise, text and labels with ONE box moved by (dx, dy) pixels
// (b).  attngan/layoutshift.py holds the definition and the numpy oracle (sums_numpy); the reference repository has no code for it.
// Everything after the fp32 loads is fp64.
//
// One workgroup per pair, so a pair's arithmetic does not depend on where in the batch it stands or on how large the batch is, and
// there is no workspace.  The S x S plane, read as one row of S S pixels, is cut into groups of four consecutive pixels; thread t owns
// the groups t, t + NT, t + 2 NT, ... in that order and a group's pixels in ascending order.  Where S S is a multiple of four and
// both images are 16-byte aligned a group of a channel is ONE 16-byte load per image, else four 4-byte loads: the values and the
// order of the arithmetic are the same, so the bits do not depend on the alignment.  A pixel's class is
//     0 old rectangle only    1 new rectangle only (old + (dx, dy))    2 both    3 neither, inside another object's rectangle    4 rest
// and the thread adds d = sum_c ((double) a - (double) b)^2 (c ascending) to the class's partial -- written as five selects
// `acc[k] += cls == k ? d : 0.0`, which keeps the partials in registers; x + 0.0 = x bit for bit for these sums of squares (never
// -0.0).  For a pixel p of the old rectangle the same thread also adds, c ascending,
//     moved    += ((double) a[p] - (double) b[p + delta])^2        baseline += ((double) a[p] - (double) a[p + delta])^2
// -- ONE expression, so b a bit copy of a gives moved == baseline bit for bit, and delta = 0 gives baseline == 0.0.  The NT threads'
// seven doubles and five counts are then added in LDS in a fixed binary tree.  No atomics.  (a - b)^2 == (b - a)^2 in IEEE
// arithmetic, so exchanging a and b changes no bit of the five class sums.
//
// A row the host should never send -- an edit rectangle that is empty or not inside the image, or whose shifted copy is not inside
// it -- is answered with zeros in all twelve outputs before any image data is read: p + delta is inside the image for every pixel of
// every rectangle that is read.  Rectangles of other objects are clipped by the class test itself (a pixel is compared against
// them, nothing is indexed by them).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

namespace {

constexpr int NT = 512;
constexpr int C_MAX = 4, S_MIN = 2, S_MAX = 1024, G_MAX = 8;
constexpr int NS = 7, NC = 5;                  // sums and counts per pair
constexpr int PX = 4;                          // consecutive pixels a thread takes at a time
constexpr long long I31 = 2147483647LL;

__global__ __launch_bounds__(NT) void box_shift_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, int C, int S,
                                                            const int* __restrict__ edit, const int* __restrict__ others, int G,
                                                            int vec, double* __restrict__ sums, int* __restrict__ counts) {
    __shared__ double red[NS][NT];
    __shared__ int redc[NC][NT];
    __shared__ int orect[G_MAX][4];
    const int tid = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int* e = edit + pair * 6;
    const int x0 = e[0], y0 = e[1], x1 = e[2], y1 = e[3], dx = e[4], dy = e[5];
    // the legality of an edit row, as attngan/layoutshift._row_ok (the oracle) and hip/ops.box_shift_sums (the host gate) state it;
    // long long: a wild offset must not wrap the test that keeps every read inside the image
    const bool ok = x0 >= 0 && y0 >= 0 && x1 > x0 && y1 > y0 && x1 <= S && y1 <= S
        && (long long)x0 + dx >= 0 && (long long)y0 + dy >= 0 && (long long)x1 + dx <= S && (long long)y1 + dy <= S;
    if (!ok) {                                                      // uniform over the workgroup: nobody reaches a barrier
        if (tid < NS) sums[pair * NS + tid] = 0.0;
        if (tid < NC) counts[pair * NC + tid] = 0;
        return;
    }
    if (tid < G * 4) orect[tid >> 2][tid & 3] = others[pair * (size_t)G * 4 + tid];
    __syncthreads();
    const size_t plane = (size_t)S * S;
    const float* pa = a + pair * (size_t)C * plane;
    const float* pb = b + pair * (size_t)C * plane;
    const int shift = dy * S + dx;
    double acc[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt[NC] = {0, 0, 0, 0, 0};
    const int n_pixels = (int)plane, groups = (n_pixels + PX - 1) / PX;
    for (int g = tid; g < groups; g += NT) {
        const int p0 = g * PX;
        // the group's loads first: four pixels of every channel of both images, as one 16-byte load each where the host found it legal
        float va[C_MAX][PX], vb[C_MAX][PX];
#pragma unroll
        for (int c = 0; c < C_MAX; ++c) {
            if (c >= C) break;
            if (vec) {
                const float4 fa = *reinterpret_cast<const float4*>(pa + c * plane + p0);
                const float4 fb = *reinterpret_cast<const float4*>(pb + c * plane + p0);
                va[c][0] = fa.x; va[c][1] = fa.y; va[c][2] = fa.z; va[c][3] = fa.w;
                vb[c][0] = fb.x; vb[c][1] = fb.y; vb[c][2] = fb.z; vb[c][3] = fb.w;
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const bool in = p0 + k < n_pixels;
                    va[c][k] = in ? pa[c * plane + p0 + k] : 0.f;
                    vb[c][k] = in ? pb[c * plane + p0 + k] : 0.f;
                }
            }
        }
        int y = p0 / S, x = p0 - y * S;                             // one division per group; the pixels after it step and wrap
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const int p = p0 + k;
            if (p < n_pixels) {
                const bool in_old = x >= x0 && x < x1 && y >= y0 && y < y1;
                const bool in_new = x >= x0 + dx && x < x1 + dx && y >= y0 + dy && y < y1 + dy;
                int cls = in_old ? (in_new ? 2 : 0) : (in_new ? 1 : 4);
                if (cls == 4) {
                    for (int o = 0; o < G; ++o)
                        if (orect[o][2] > orect[o][0] && x >= orect[o][0] && x < orect[o][2] && y >= orect[o][1] && y < orect[o][3]) cls = 3;
                }
                const int ps = in_old ? p + shift : p;              // inside the plane: the shifted rectangle is inside the image
                double d = 0.0;
#pragma unroll
                for (int c = 0; c < C_MAX; ++c) {
                    if (c >= C) break;
                    const double a_p = (double)va[c][k];
                    const double t = a_p - (double)vb[c][k];
                    d += t * t;
                    if (in_old) {
                        const double m = a_p - (double)pb[c * plane + ps];
                        const double q = a_p - (double)pa[c * plane + ps];
                        acc[5] += m * m;
                        acc[6] += q * q;
                    }
                }
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    acc[j] += cls == j ? d : 0.0;
                    cnt[j] += cls == j ? 1 : 0;
                }
            }
            if (++x == S) { x = 0; ++y; }
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][tid] = acc[k];
#pragma unroll
    for (int k = 0; k < NC; ++k) redc[k][tid] = cnt[k];
    __syncthreads();
    for (int off = NT / 2; off >= 1; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k][tid] += red[k][tid + off];
#pragma unroll
            for (int k = 0; k < NC; ++k) redc[k][tid] += redc[k][tid + off];
        }
        __syncthreads();
    }
    if (tid < NS) sums[pair * NS + tid] = red[tid][0];
    if (tid < NC) counts[pair * NC + tid] = redc[tid][0];
}

}  // namespace

extern "C" {

int mogan_box_shift_sums_f64(const float* a, const float* b, long long P, int C, int S, const int* edit, const int* others, int G,
                             double* sums, int* counts, hipStream_t stream) {
    if (!a || !b || !edit || !sums || !counts || P < 1 || C < 1 || C > C_MAX || S < S_MIN || S > S_MAX || G < 0 || G > G_MAX)
        return MOGAN_ERR_SHAPE;
    if (G > 0 && !others) return MOGAN_ERR_SHAPE;
    if (P > I31 / ((long long)C * S * S)) return MOGAN_ERR_SHAPE;                                // P C S S <= 2^31 - 1
    // 16-byte loads: every channel plane of every pair then starts on a 16-byte boundary and holds whole groups
    const int vec = ((long long)S * S) % PX == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    hipLaunchKernelGGL(box_shift_sums_kernel, dim3((unsigned)P), dim3(NT), 0, stream, a, b, C, S, edit, others, G, vec, sums, counts);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

}  // extern "C"
