// mogan_stn_attn.hip -- the two ops that are specific to this repo's generator/discriminators:
//
//  * stn: the "object pathway" spatial transformer (code/coco/attngan/model.py:17-21):
//    affine_grid(theta) + grid_sample(bilinear, zero padding).  bbox = -1 (absent object) gives
//    theta_inv = [[-1,0,-4],[0,-1,-4]] whose grid lies wholly outside [-1,1] -> exactly 0.
//    HBM-bound gather; one thread per output pixel loops over the channels (the 4 taps and weights
//    depend only on (b,oy,ox)), so consecutive lanes read consecutive x of the same plane.
//  * GlobalAttentionGeneral core (GlobalAttention.py:96-121): per query pixel q, scores over the
//    T <= 32 words (K = idf <= 128), masked softmax, weighted context.  One thread per query; the
//    (idf x T) word projection sits in LDS and is read as broadcasts; h is read and wc/attn written
//    with q contiguous across lanes.  T is tiny: no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

namespace {

static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

// the kernels index a plane with ints and the grids round it up to blocks of 256: Hin * Win and Hout * Wout stay 256 below 2^31
static inline bool plane_fits(int H, int W) { return (long long)H * W <= 0x7fffffffLL - 255; }

// channel chunks per sample of the forward, so that about 1024 blocks run (pb * B may pass an int: counted in 64 bits)
static inline int stn_csplit(int pb, int B, int C) {
    const long long blocks = (long long)pb * B;
    long long csplit = (1024 + blocks - 1) / blocks;
    if (csplit > C) csplit = C;
    return csplit < 1 ? 1 : (int)csplit;
}

struct Taps { int x0, y0; float wx1, wy1; bool vx0, vx1, vy0, vy1; };

__device__ __forceinline__ Taps stn_taps(const float* __restrict__ th, int oy, int ox, int Hin, int Win, int Hout,
                                         int Wout, int ac) {
    float xn, yn;
    if (ac) {
        xn = Wout > 1 ? 2.f * ox / (float)(Wout - 1) - 1.f : 0.f;
        yn = Hout > 1 ? 2.f * oy / (float)(Hout - 1) - 1.f : 0.f;
    } else {
        xn = (2.f * ox + 1.f) / (float)Wout - 1.f;
        yn = (2.f * oy + 1.f) / (float)Hout - 1.f;
    }
    const float gx = th[0] * xn + th[1] * yn + th[2];
    const float gy = th[3] * xn + th[4] * yn + th[5];
    float ix, iy;
    if (ac) { ix = (gx + 1.f) * 0.5f * (float)(Win - 1); iy = (gy + 1.f) * 0.5f * (float)(Hin - 1); }
    else { ix = ((gx + 1.f) * (float)Win - 1.f) * 0.5f; iy = ((gy + 1.f) * (float)Hin - 1.f) * 0.5f; }
    Taps t;
    const float fx = floorf(ix), fy = floorf(iy);
    // clamp before the int conversion so wild thetas (absent objects) cannot overflow
    t.x0 = (int)fminf(fmaxf(fx, -2.f), (float)Win + 1.f);
    t.y0 = (int)fminf(fmaxf(fy, -2.f), (float)Hin + 1.f);
    t.wx1 = ix - fx; t.wy1 = iy - fy;
    const bool inx = (fx >= -1.f && fx <= (float)Win), iny = (fy >= -1.f && fy <= (float)Hin);
    t.vx0 = inx && t.x0 >= 0 && t.x0 < Win; t.vx1 = inx && t.x0 + 1 >= 0 && t.x0 + 1 < Win;
    t.vy0 = iny && t.y0 >= 0 && t.y0 < Hin; t.vy1 = iny && t.y0 + 1 >= 0 && t.y0 + 1 < Hin;
    return t;
}

// shared / constant sources (mogan_stn_*_ex): output sample b reads image b % xB; PLANE: x is (xB, C), constant over the plane
template <bool PLANE>
__global__ __launch_bounds__(256) void stn_fwd_ex_kernel(const float* __restrict__ x, const float* __restrict__ theta,
                                                         float* __restrict__ y, int C, int Hin, int Win, int Hout,
                                                         int Wout, int ac, int cchunk, int xB, int tG) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hout * Wout) return;
    const int b = blockIdx.z, bx = b % xB, c0 = blockIdx.y * cchunk, c1 = min(C, c0 + cchunk);
    const int oy = pix / Wout, ox = pix - oy * Wout;
    // tG > 0: theta is stored (B', tG, 2, 3) and sample b = g B' + b' (object-major batch) uses theta[b'][g]
    const int nb = tG > 0 ? (int)gridDim.z / tG : 1;
    const int tb = tG > 0 ? (b % nb) * tG + b / nb : b;
    const Taps t = stn_taps(theta + tb * 6, oy, ox, Hin, Win, Hout, Wout, ac);
    const float w00 = (1.f - t.wx1) * (1.f - t.wy1), w01 = t.wx1 * (1.f - t.wy1);
    const float w10 = (1.f - t.wx1) * t.wy1, w11 = t.wx1 * t.wy1;
    const bool v00 = t.vx0 && t.vy0, v01 = t.vx1 && t.vy0, v10 = t.vx0 && t.vy1, v11 = t.vx1 && t.vy1;
    const int o00 = t.y0 * Win + t.x0;
    for (int c = c0; c < c1; ++c) {
        float acc = 0.f;
        if (PLANE) {                       // the same four products in the same order as on the materialised plane
            const float v = x[(size_t)bx * C + c];
            if (v00) acc += v * w00;
            if (v01) acc += v * w01;
            if (v10) acc += v * w10;
            if (v11) acc += v * w11;
        } else {
            const float* px = x + ((size_t)bx * C + c) * Hin * Win;
            if (v00) acc += px[o00] * w00;
            if (v01) acc += px[o00 + 1] * w01;
            if (v10) acc += px[o00 + Win] * w10;
            if (v11) acc += px[o00 + Win + 1] * w11;
        }
        y[((size_t)b * C + c) * Hout * Wout + pix] = acc;
    }
}

// Backward as a gather in a fixed order (bit-reproducible, no atomics): dx of source pixel (bx, c, sy, sx) collects, for the
// samples b = bx, bx + xB, ... in order and their output pixels in row-major order, dy * the weight of every tap of that
// output pixel that lands on (sx, sy).  The taps are those of the forward (stn_taps); the output pixels searched are the
// preimage window of the source cell [sx-1, sx+1) x [sy-1, sy+1) under theta, widened by 1 pixel (a singular theta or a
// one-pixel source axis searches the whole output).
struct Win2 { int x0, x1, y0, y1; };

__device__ __forceinline__ Win2 stn_preimage(const float* __restrict__ th, int sy, int sx, int Hin, int Win, int Hout,
                                             int Wout, int ac) {
    Win2 w = {0, Wout - 1, 0, Hout - 1};
    const double a = th[0], bb = th[1], tx = th[2], c = th[3], d = th[4], ty = th[5];
    const double det = a * d - bb * c;
    if (!(fabs(det) > 1e-30) || (ac && (Win < 2 || Hin < 2))) return w;
    double lox = 1e300, hix = -1e300, loy = 1e300, hiy = -1e300;
    for (int k = 0; k < 4; ++k) {
        const double ix = sx - 1 + 2 * (k & 1), iy = sy - 1 + 2 * (k >> 1);      // corners of the source cell
        const double gx = ac ? 2.0 * ix / (Win - 1) - 1.0 : (2.0 * ix + 1.0) / Win - 1.0;
        const double gy = ac ? 2.0 * iy / (Hin - 1) - 1.0 : (2.0 * iy + 1.0) / Hin - 1.0;
        const double xn = (d * (gx - tx) - bb * (gy - ty)) / det, yn = (a * (gy - ty) - c * (gx - tx)) / det;
        const double ox = ac ? (xn + 1.0) * 0.5 * (Wout - 1) : ((xn + 1.0) * Wout - 1.0) * 0.5;
        const double oy = ac ? (yn + 1.0) * 0.5 * (Hout - 1) : ((yn + 1.0) * Hout - 1.0) * 0.5;
        lox = fmin(lox, ox); hix = fmax(hix, ox); loy = fmin(loy, oy); hiy = fmax(hiy, oy);
    }
    if (!(lox <= hix && loy <= hiy)) return w;                               // non-finite theta: search everything
    // clamped to [-1, W] before the int conversion (an empty window when the preimage misses the output)
    w.x0 = (int)fmin(fmax(floor(lox) - 1.0, 0.0), (double)Wout); w.x1 = (int)fmax(fmin(ceil(hix) + 1.0, (double)(Wout - 1)), -1.0);
    w.y0 = (int)fmin(fmax(floor(loy) - 1.0, 0.0), (double)Hout); w.y1 = (int)fmax(fmin(ceil(hiy) + 1.0, (double)(Hout - 1)), -1.0);
    return w;
}

// weight of output pixel (oy, ox)'s taps on source pixel (sy, sx), summed in the forward's tap order
__device__ __forceinline__ float stn_tap_weight(const Taps& t, int sy, int sx) {
    float w = 0.f;
    const bool x0 = t.x0 == sx, x1 = t.x0 + 1 == sx, y0 = t.y0 == sy, y1 = t.y0 + 1 == sy;
    if (x0 && y0 && t.vx0 && t.vy0) w += (1.f - t.wx1) * (1.f - t.wy1);
    if (x1 && y0 && t.vx1 && t.vy0) w += t.wx1 * (1.f - t.wy1);
    if (x0 && y1 && t.vx0 && t.vy1) w += (1.f - t.wx1) * t.wy1;
    if (x1 && y1 && t.vx1 && t.vy1) w += t.wx1 * t.wy1;
    return w;
}

constexpr int STN_BWD_CC = 8;              // channels per thread of the gather (its accumulators)

// grid (ceil(Hin Win / 256), ceil(C / STN_BWD_CC), xB); B samples, sample b reads image b % xB; tG as in stn_fwd_ex_kernel
__global__ __launch_bounds__(256) void stn_bwd_gather_kernel(const float* __restrict__ dy, const float* __restrict__ theta,
                                                             float* __restrict__ dx, int B, int C, int Hin, int Win,
                                                             int Hout, int Wout, int ac, int xB, int tG) {
    const int sp = blockIdx.x * 256 + threadIdx.x;
    if (sp >= Hin * Win) return;
    const int bx = blockIdx.z, c0 = blockIdx.y * STN_BWD_CC, nc = min(C - c0, STN_BWD_CC);
    const int sy = sp / Win, sx = sp - sy * Win;
    const int nb = tG > 0 ? B / tG : 1;
    float acc[STN_BWD_CC];
#pragma unroll
    for (int k = 0; k < STN_BWD_CC; ++k) acc[k] = 0.f;
    for (int b = bx; b < B; b += xB) {
        const int tb = tG > 0 ? (b % nb) * tG + b / nb : b;
        const float* th = theta + tb * 6;
        const Win2 w = stn_preimage(th, sy, sx, Hin, Win, Hout, Wout, ac);
        const float* g = dy + ((size_t)b * C + c0) * Hout * Wout;
        for (int oy = w.y0; oy <= w.y1; ++oy)
            for (int ox = w.x0; ox <= w.x1; ++ox) {
                const float wt = stn_tap_weight(stn_taps(th, oy, ox, Hin, Win, Hout, Wout, ac), sy, sx);
                if (wt == 0.f) continue;
                const size_t o = (size_t)oy * Wout + ox;
#pragma unroll
                for (int k = 0; k < STN_BWD_CC; ++k)
                    if (k < nc) acc[k] += g[(size_t)k * Hout * Wout + o] * wt;
            }
    }
#pragma unroll
    for (int k = 0; k < STN_BWD_CC; ++k)
        if (k < nc) dx[((size_t)bx * C + c0 + k) * Hin * Win + sp] = acc[k];
}

// x_plane: d x[bx, c] = sum over the samples b = bx, bx + xB, ... and their output pixels of dy * (sum of the in-range tap
// weights); one block per (c, bx), each thread a fixed strided subset, then a fixed-shape tree in LDS
__global__ __launch_bounds__(256) void stn_bwd_plane_kernel(const float* __restrict__ dy, const float* __restrict__ theta,
                                                            float* __restrict__ dx, int B, int C, int Hin, int Win,
                                                            int Hout, int Wout, int ac, int xB, int tG) {
    __shared__ float red[256];
    const int c = blockIdx.x, bx = blockIdx.y, HW = Hout * Wout;
    const int nb = tG > 0 ? B / tG : 1;
    float acc = 0.f;
    for (int b = bx; b < B; b += xB) {
        const int tb = tG > 0 ? (b % nb) * tG + b / nb : b;
        const float* g = dy + ((size_t)b * C + c) * HW;
        for (int pix = threadIdx.x; pix < HW; pix += 256) {
            const int oy = pix / Wout, ox = pix - oy * Wout;
            const Taps t = stn_taps(theta + tb * 6, oy, ox, Hin, Win, Hout, Wout, ac);
            const float w00 = (1.f - t.wx1) * (1.f - t.wy1), w01 = t.wx1 * (1.f - t.wy1);
            const float w10 = (1.f - t.wx1) * t.wy1, w11 = t.wx1 * t.wy1;
            const float wsum = (t.vx0 && t.vy0 ? w00 : 0.f) + (t.vx1 && t.vy0 ? w01 : 0.f) +
                               (t.vx0 && t.vy1 ? w10 : 0.f) + (t.vx1 && t.vy1 ? w11 : 0.f);
            acc += g[pix] * wsum;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) dx[(size_t)bx * C + c] = red[0];
}

__global__ __launch_bounds__(256) void stn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ theta,
                                                      float* __restrict__ y, int C, int Hin, int Win, int Hout,
                                                      int Wout, int ac, int cchunk) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hout * Wout) return;
    const int b = blockIdx.z, c0 = blockIdx.y * cchunk, c1 = min(C, c0 + cchunk);
    const int oy = pix / Wout, ox = pix - oy * Wout;
    const Taps t = stn_taps(theta + b * 6, oy, ox, Hin, Win, Hout, Wout, ac);
    const float w00 = (1.f - t.wx1) * (1.f - t.wy1), w01 = t.wx1 * (1.f - t.wy1);
    const float w10 = (1.f - t.wx1) * t.wy1, w11 = t.wx1 * t.wy1;
    const bool v00 = t.vx0 && t.vy0, v01 = t.vx1 && t.vy0, v10 = t.vx0 && t.vy1, v11 = t.vx1 && t.vy1;
    const int o00 = t.y0 * Win + t.x0;
    for (int c = c0; c < c1; ++c) {
        const float* px = x + ((size_t)b * C + c) * Hin * Win;
        float acc = 0.f;
        if (v00) acc += px[o00] * w00;
        if (v01) acc += px[o00 + 1] * w01;
        if (v10) acc += px[o00 + Win] * w10;
        if (v11) acc += px[o00 + Win + 1] * w11;
        y[((size_t)b * C + c) * Hout * Wout + pix] = acc;
    }
}

__global__ void bbox_to_theta_kernel(const float* __restrict__ bbox, float* __restrict__ th, float* __restrict__ thi,
                                     int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float x = bbox[i * 4], y = bbox[i * 4 + 1], w = bbox[i * 4 + 2], h = bbox[i * 4 + 3];
    // same operation order as miscc/utils.py:16-49, no fma contraction
    const float cx = __fadd_rn(x, __fmul_rn(0.5f, w)), cy = __fadd_rn(y, __fmul_rn(0.5f, h));
    float* t = th + i * 6;
    t[0] = w; t[1] = 0.f; t[2] = __fmul_rn(2.f, __fsub_rn(cx, 0.5f));
    t[3] = 0.f; t[4] = h; t[5] = __fmul_rn(2.f, __fsub_rn(cy, 0.5f));
    const float sx = __fdiv_rn(1.0f, w), sy = __fdiv_rn(1.0f, h);
    float* u = thi + i * 6;
    u[0] = sx; u[1] = 0.f; u[2] = __fmul_rn(__fmul_rn(2.f, sx), __fsub_rn(0.5f, cx));
    u[3] = 0.f; u[4] = sy; u[5] = __fmul_rn(__fmul_rn(2.f, sy), __fsub_rn(0.5f, cy));
}

// ------------------------------------------------------------------------------------ attention
// Round 4: the word projections sit in LDS zero-padded to TMAX slots per channel and every multiply-add loop runs over all
// TMAX slots -- the `t < T` tests of the earlier form were uniform branches inside the unrolled loops, which left one global
// load and a dozen FMAs per basic block with nothing in flight between them (61 us per launch against a 20 us HBM bound); the
// channel loops now issue eight loads before their multiplies.
template <int TMAX>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ h, const float* __restrict__ src,
                                                       const uint8_t* __restrict__ mask, float* __restrict__ wc,
                                                       float* __restrict__ attn, int B, int idf, int Q, int T,
                                                       int mask_mode) {
    extern __shared__ __attribute__((aligned(16))) float s_src[];     // [idf][TMAX], slots >= T are zero
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < idf * TMAX; i += 256) {
        const int c = i / TMAX, t = i - c * TMAX;
        s_src[i] = t < T ? src[((size_t)b * idf + c) * T + t] : 0.f;
    }
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    float s[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) s[t] = 0.f;
    const float* ph = h + (size_t)b * idf * Q + q;
    int c = 0;
    for (; c + 8 <= idf; c += 8) {
        float hv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) hv[u] = ph[(size_t)(c + u) * Q];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int t = 0; t < TMAX; ++t) s[t] = fmaf(hv[u], s_src[(c + u) * TMAX + t], s[t]);
    }
    for (; c < idf; ++c) {
        const float hv = ph[(size_t)c * Q];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) s[t] = fmaf(hv, s_src[c * TMAX + t], s[t]);
    }
    // reference: mask.repeat(queryL,1) laid over rows b*Q+q  ->  row r uses mask[r % B]  
    const uint8_t* pm = nullptr;
    if (mask) pm = mask + (size_t)(mask_mode == 0 ? (int)(((long long)b * Q + q) % B) : b) * T;
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        bool off = t >= T;
        if (t < T && pm != nullptr && pm[t] != 0) off = true;
        if (off) s[t] = -INFINITY;
        m = fmaxf(m, s[t]);
    }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) { s[t] = __expf(s[t] - m); sum += s[t]; }     // (slots >= T: exp(-inf) = 0)
    const float inv = 1.f / sum;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) { s[t] *= inv; if (t < T) attn[((size_t)b * T + t) * Q + q] = s[t]; }
    float* pw = wc + (size_t)b * idf * Q + q;
    for (int c2 = 0; c2 < idf; ++c2) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) a = fmaf(s_src[c2 * TMAX + t], s[t], a);
        pw[(size_t)c2 * Q] = a;
    }
}

// dp[t] = sum_c dwc[c,q]*src[c,t] (+dattn[t,q]); ds = p*(dp - sum p*dp); dh[c,q] = sum_t ds[t]*src[c,t]
template <int TMAX>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ src, const float* __restrict__ attn,
                                                       const float* __restrict__ dwc, const float* __restrict__ dattn,
                                                       float* __restrict__ dh, float* __restrict__ dscore, int idf,
                                                       int Q, int T) {
    extern __shared__ __attribute__((aligned(16))) float s_src[];     // [idf][TMAX], slots >= T are zero
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < idf * TMAX; i += 256) {
        const int c = i / TMAX, t = i - c * TMAX;
        s_src[i] = t < T ? src[((size_t)b * idf + c) * T + t] : 0.f;
    }
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    float dp[TMAX], p[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        p[t] = t < T ? attn[((size_t)b * T + t) * Q + q] : 0.f;
        dp[t] = (t < T && dattn) ? dattn[((size_t)b * T + t) * Q + q] : 0.f;
    }
    const float* pd = dwc + (size_t)b * idf * Q + q;
    int c = 0;
    for (; c + 8 <= idf; c += 8) {
        float gv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) gv[u] = pd[(size_t)(c + u) * Q];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int t = 0; t < TMAX; ++t) dp[t] = fmaf(gv[u], s_src[(c + u) * TMAX + t], dp[t]);
    }
    for (; c < idf; ++c) {
        const float g = pd[(size_t)c * Q];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) dp[t] = fmaf(g, s_src[c * TMAX + t], dp[t]);
    }
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) dot = fmaf(p[t], dp[t], dot);           // (p = 0 in the slots >= T)
#pragma unroll
    for (int t = 0; t < TMAX; ++t) { dp[t] = p[t] * (dp[t] - dot); if (t < T) dscore[((size_t)b * T + t) * Q + q] = dp[t]; }
    float* po = dh + (size_t)b * idf * Q + q;
    for (int c2 = 0; c2 < idf; ++c2) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) a = fmaf(dp[t], s_src[c2 * TMAX + t], a);
        po[(size_t)c2 * Q] = a;
    }
}

}  // namespace

extern "C" {

int mogan_stn_fwd(const float* x, const float* theta, float* y, int B, int C, int Hin, int Win, int Hout, int Wout,
                  int align_corners, hipStream_t stream) {
    if (!x || !theta || !y) return MOGAN_ERR_SHAPE;
    if (B <= 0 || C <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || B > 65535) return MOGAN_ERR_SHAPE;
    if (!plane_fits(Hin, Win) || !plane_fits(Hout, Wout)) return MOGAN_ERR_SHAPE;
    const int pb = (Hout * Wout + 255) / 256;
    int csplit = stn_csplit(pb, B, C);
    const int cchunk = (C + csplit - 1) / csplit; csplit = (C + cchunk - 1) / cchunk;
    hipLaunchKernelGGL(stn_fwd_kernel, dim3(pb, csplit, B), dim3(256), 0, stream, x, theta, y, C, Hin, Win, Hout, Wout,
                       align_corners, cchunk);
    return ok_launch();
}

int mogan_stn_bwd(const float* dy, const float* theta, float* dx, int B, int C, int Hin, int Win, int Hout,
                  int Wout, int align_corners, hipStream_t stream) {
    return mogan_stn_bwd_ex(dy, theta, dx, B, C, Hin, Win, Hout, Wout, align_corners, B, 0, 0, stream);
}

int mogan_stn_fwd_ex(const float* x, const float* theta, float* y, int B, int C, int Hin, int Win, int Hout, int Wout,
                     int align_corners, int xB, int x_plane, int theta_G, hipStream_t stream) {
    if (B <= 0 || C <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || B > 65535 || xB <= 0 || B % xB != 0 ||
        theta_G < 0 || (theta_G > 0 && B % theta_G != 0))
        return MOGAN_ERR_SHAPE;
    if (!x || !theta || !y || !plane_fits(Hin, Win) || !plane_fits(Hout, Wout)) return MOGAN_ERR_SHAPE;
    const int pb = (Hout * Wout + 255) / 256;
    int csplit = stn_csplit(pb, B, C);
    const int cchunk = (C + csplit - 1) / csplit; csplit = (C + cchunk - 1) / cchunk;
    if (x_plane) hipLaunchKernelGGL((stn_fwd_ex_kernel<true>), dim3(pb, csplit, B), dim3(256), 0, stream, x, theta, y, C, Hin, Win,
                                    Hout, Wout, align_corners, cchunk, xB, theta_G);
    else hipLaunchKernelGGL((stn_fwd_ex_kernel<false>), dim3(pb, csplit, B), dim3(256), 0, stream, x, theta, y, C, Hin, Win,
                            Hout, Wout, align_corners, cchunk, xB, theta_G);
    return ok_launch();
}

int mogan_stn_bwd_ex(const float* dy, const float* theta, float* dx, int B, int C, int Hin, int Win, int Hout, int Wout,
                     int align_corners, int xB, int x_plane, int theta_G, hipStream_t stream) {
    if (B <= 0 || C <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || B > 65535 || xB <= 0 || B % xB != 0 ||
        theta_G < 0 || (theta_G > 0 && B % theta_G != 0))
        return MOGAN_ERR_SHAPE;
    if (!dy || !theta || !dx || !plane_fits(Hin, Win) || !plane_fits(Hout, Wout)) return MOGAN_ERR_SHAPE;
    if (x_plane) {
        hipLaunchKernelGGL(stn_bwd_plane_kernel, dim3(C, xB), dim3(256), 0, stream, dy, theta, dx, B, C, Hin, Win, Hout, Wout,
                           align_corners, xB, theta_G);
    } else {
        const int cg = (C + STN_BWD_CC - 1) / STN_BWD_CC;
        if (cg > 65535) return MOGAN_ERR_SHAPE;
        hipLaunchKernelGGL(stn_bwd_gather_kernel, dim3((Hin * Win + 255) / 256, cg, xB), dim3(256), 0, stream, dy, theta, dx,
                           B, C, Hin, Win, Hout, Wout, align_corners, xB, theta_G);
    }
    return ok_launch();
}

int mogan_bbox_to_theta(const float* bbox, float* theta, float* theta_inv, int N, hipStream_t stream) {
    if (N <= 0 || !bbox || !theta || !theta_inv) return MOGAN_ERR_SHAPE;
    hipLaunchKernelGGL(bbox_to_theta_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, bbox, theta, theta_inv, N);
    return ok_launch();
}

int mogan_attn_fwd(const float* h, const float* src, const uint8_t* mask, float* wc, float* attn, int B, int idf,
                   int Q, int T, int mask_mode, hipStream_t stream) {
    if (B <= 0 || idf <= 0 || idf > 128 || Q <= 0 || T <= 0 || T > 32 || B > 65535) return MOGAN_ERR_SHAPE;
    if (!h || !src || !wc || !attn) return MOGAN_ERR_SHAPE;                  // (mask is nullable)
    dim3 grid((Q + 255) / 256, B);
    const size_t sh = (size_t)idf * (T <= 8 ? 8 : T <= 16 ? 16 : 32) * sizeof(float);
    if (T <= 8) hipLaunchKernelGGL((attn_fwd_kernel<8>), grid, dim3(256), sh, stream, h, src, mask, wc, attn, B, idf, Q, T, mask_mode);
    else if (T <= 16) hipLaunchKernelGGL((attn_fwd_kernel<16>), grid, dim3(256), sh, stream, h, src, mask, wc, attn, B, idf, Q, T, mask_mode);
    else hipLaunchKernelGGL((attn_fwd_kernel<32>), grid, dim3(256), sh, stream, h, src, mask, wc, attn, B, idf, Q, T, mask_mode);
    return ok_launch();
}

int mogan_attn_bwd(const float* src, const float* attn, const float* dwc, const float* dattn, float* dh,
                   float* dscore, int B, int idf, int Q, int T, hipStream_t stream) {
    if (B <= 0 || idf <= 0 || idf > 128 || Q <= 0 || T <= 0 || T > 32 || B > 65535) return MOGAN_ERR_SHAPE;
    if (!src || !attn || !dwc || !dh || !dscore) return MOGAN_ERR_SHAPE;     // (dattn is nullable)
    dim3 grid((Q + 255) / 256, B);
    const size_t sh = (size_t)idf * (T <= 8 ? 8 : T <= 16 ? 16 : 32) * sizeof(float);
    if (T <= 8) hipLaunchKernelGGL((attn_bwd_kernel<8>), grid, dim3(256), sh, stream, src, attn, dwc, dattn, dh, dscore, idf, Q, T);
    else if (T <= 16) hipLaunchKernelGGL((attn_bwd_kernel<16>), grid, dim3(256), sh, stream, src, attn, dwc, dattn, dh, dscore, idf, Q, T);
    else hipLaunchKernelGGL((attn_bwd_kernel<32>), grid, dim3(256), sh, stream, src, attn, dwc, dattn, dh, dscore, idf, Q, T);
    return ok_launch();
}

}  // extern "C"
