// mogan_gru.hip -- the text encoder with cfg.RNN_TYPE = 'GRU': the eval forward as ONE launch, the training forward and
// back-propagation through time of DAMSM pre-training as one launch each.  The layout is mogan_lstm.hip's with three gate rows per
// unit instead of four; the embedding gradient (mogan_embedding_bwd) and the weight-gradient GEMMs (mogan_bmm) are shared.
//
// RNN_ENCODER (code/coco/attngan/model.py:120-204) with nn.GRU: one layer, bidirectional, H = 128 units per direction, PyTorch's gate
// order r, z, n:
//   r = s(W_ir x + b_ir + W_hr h + b_hr)      z = s(W_iz x + b_iz + W_hz h + b_hz)
//   hn = W_hn h + b_hn                        n = tanh(W_in x + b_in + r * hn)            h' = (1 - z) * n + z * h
// A block owns one (direction, caption):
//   * 384 threads = the 384 gate rows.  The embedded caption sits in LDS (<= 40 KiB); thread j streams row j of W_ih ONCE, forms its
//     input projection for every time step in registers and parks it in LDS [t][384] (<= 48 KiB).  The r and z rows fold b_ih + b_hh
//     into it; the n rows fold b_ih only, because b_hn sits inside r * (...),
//   * then holds row j of W_hh (128 values) in registers for the recurrence: per step 128 fmas against the hidden state in LDS
//     (broadcast reads); the r / z rows hand over their full pre-activation, the n rows hand over hn; the 128 unit threads apply the
//     gates, write h into the output row of step t and back to LDS; two barriers per step.
// The reverse direction walks t = len - 1 ... 0; positions t >= len of words are written as zeros (pad_packed_sequence).
// fp32 throughout, expf / tanhf (no fast-math forms), no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"
#include "mogan_internal.h"

namespace {

constexpr int GR_H = 128, GR_G = 3 * GR_H, GR_TMAX = 32, GR_EMAX = 320, GR_BMAX = 64;

struct GruP {
    const long long* cap; const float* emb;
    const float* w_ih[2]; const float* w_hh[2]; const float* b_ih[2]; const float* b_hh[2];
    const float* h0;
    float* words; float* sent;
    // training only (all NULL / 1 in the eval kernel): embedding dropout and what back-propagation needs
    const uint8_t* mask; float scale;
    float* x; float* gates; float* hn; float* hprev;
    int B, T, Tmax, V, E;
    int lens[GR_BMAX];
};

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// TRAIN = false: the eval forward.  TRAIN = true: the same arithmetic with the embedding row * (keep ? scale : 0) and the saved
// tensors written on the way: x (the masked, scaled rows; by the forward direction's block), the post-activation gates r, z, n, hn,
// and the hidden state that entered each step; all zero at t >= len.
template <bool TRAIN>
__global__ __launch_bounds__(GR_G) void gru_encoder_kernel(const GruP p) {
    // one array, the recurrence's small buffers first: their reads then fit the LDS instructions' 16-bit immediate offsets (behind
    // the 88 KiB of Xs / XP every one of the 32 reads of Hs per step would need an address register of its own: scratch)
    __shared__ __attribute__((aligned(16))) float smem[GR_H + GR_G + GR_TMAX * GR_G + GR_TMAX * GR_EMAX];
    float* const Hs = smem;                                      // the hidden state
    float* const Gs = Hs + GR_H;                                 // r, z pre-activations and hn of the step
    float* const XP = Gs + GR_G;                                 // input projections [t][gate row]
    float* const Xs = XP + GR_TMAX * GR_G;                       // the embedded caption [t][E]
    const int j = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int E = p.E, len = min(max(p.lens[b], 0), p.Tmax);
    // ---- the caption's embedding rows
    if (j < E) {
        for (int t = 0; t < (TRAIN ? p.Tmax : len); ++t) {
            float v = 0.f;
            if (t < len) {
                long long tok = p.cap[(size_t)b * p.T + t];
                tok = tok < 0 ? 0 : (tok >= p.V ? p.V - 1 : tok);
                v = p.emb[(size_t)tok * E + j];
                if (TRAIN) v *= p.mask ? (p.mask[((size_t)b * p.T + t) * E + j] ? p.scale : 0.f) : p.scale;
                Xs[t * GR_EMAX + j] = v;
            }
            if (TRAIN && dir == 0) p.x[((size_t)b * p.Tmax + t) * E + j] = v;
        }
    }
    __syncthreads();
    // ---- input projection of every step: one pass over row j of W_ih
    const float bhh = p.b_hh[dir][j];
    const bool nrow = j >= 2 * GR_H;                             // (the same for a whole wave)
    {
        float acc[GR_TMAX];
        const float bias = p.b_ih[dir][j] + (nrow ? 0.f : bhh);
#pragma unroll
        for (int t = 0; t < GR_TMAX; ++t) acc[t] = bias;
        const float4* wr = (const float4*)(p.w_ih[dir] + (size_t)j * E);
        for (int k4 = 0; k4 < E / 4; ++k4) {
            const float4 w = wr[k4];
#pragma unroll
            for (int t = 0; t < GR_TMAX; ++t)
                if (t < len) {                                   // (the same for the whole block)
                    const float4 x = *(const float4*)&Xs[t * GR_EMAX + 4 * k4];
                    acc[t] = fmaf(w.x, x.x, acc[t]); acc[t] = fmaf(w.y, x.y, acc[t]);
                    acc[t] = fmaf(w.z, x.z, acc[t]); acc[t] = fmaf(w.w, x.w, acc[t]);
                }
        }
#pragma unroll
        for (int t = 0; t < GR_TMAX; ++t) if (t < len) XP[t * GR_G + j] = acc[t];
    }
    // ---- recurrence
    float4 whh[GR_H / 4];
    {
        const float4* hr = (const float4*)(p.w_hh[dir] + (size_t)j * GR_H);
#pragma unroll
        for (int k4 = 0; k4 < GR_H / 4; ++k4) whh[k4] = hr[k4];
    }
    float h = 0.f;
    if (j < GR_H) {
        if (p.h0) h = p.h0[((size_t)dir * p.B + b) * GR_H + j];
        Hs[j] = h;
    }
    __syncthreads();
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;                    // row (dir, b, t = 0) of the saved tensors
    float* wout = p.words + ((size_t)b * 2 * GR_H + (size_t)dir * GR_H) * p.Tmax;
    for (int s = 0; s < len; ++s) {
        const int t = dir ? len - 1 - s : s;
        float a0 = nrow ? bhh : XP[t * GR_G + j], a1 = 0.f, a2 = 0.f, a3 = 0.f;   // four chains, summed at the end
#pragma unroll
        for (int k4 = 0; k4 < GR_H / 4; ++k4) {
            const float4 hv = *(const float4*)&Hs[4 * k4];
            a0 = fmaf(whh[k4].x, hv.x, a0); a1 = fmaf(whh[k4].y, hv.y, a1);
            a2 = fmaf(whh[k4].z, hv.z, a2); a3 = fmaf(whh[k4].w, hv.w, a3);
        }
        Gs[j] = (a0 + a1) + (a2 + a3);                           // r, z: the pre-activation; n rows: hn
        __syncthreads();
        if (j < GR_H) {
            const float r = sigm(Gs[j]), z = sigm(Gs[GR_H + j]), hn = Gs[2 * GR_H + j];
            const float n = tanhf(XP[t * GR_G + 2 * GR_H + j] + r * hn);
            if (TRAIN) {
                float* gr = p.gates + (base + t) * GR_G;
                gr[j] = r; gr[GR_H + j] = z; gr[2 * GR_H + j] = n;
                p.hn[(base + t) * GR_H + j] = hn;
                p.hprev[(base + t) * GR_H + j] = h;
            }
            h = (1.f - z) * n + z * h;
            Hs[j] = h;
            wout[(size_t)j * p.Tmax + t] = h;
        }
        __syncthreads();
    }
    if (j < GR_H) {
        p.sent[(size_t)b * 2 * GR_H + dir * GR_H + j] = h;
        for (int t = len; t < p.Tmax; ++t) {
            wout[(size_t)j * p.Tmax + t] = 0.f;
            if (TRAIN) { p.hn[(base + t) * GR_H + j] = 0.f; p.hprev[(base + t) * GR_H + j] = 0.f; }
        }
    }
    if (TRAIN)
        for (int t = len; t < p.Tmax; ++t) p.gates[(base + t) * GR_G + j] = 0.f;
}

// gru_encoder_bwd_kernel: back-propagation through time, one block of 384 threads per (direction, caption), walking the forward's
// steps backwards.  Per step
//   * the 128 unit threads (tid < 128) turn d h' (= d words[:, t] + the recurrent part + d sent at the walk's last step) into
//       dn = dh' (1 - z)(1 - n^2),  dz = dh' (h_prev - n) z (1 - z),  dr = dn hn r (1 - r),
//     write the input-side gradients dgi = (dr, dz, dn) and the hidden-side ones dgh = (dr, dz, dn r) (b_hn and W_hn sit inside
//     r * (...)), the latter to LDS as well (1.5 KiB), and keep dh' z,
//   * then all 384 threads form W_hh^T . dgh: thread (k = tid % 128, q = tid / 128) holds W_hh[q * 128 ... + 127][k], i.e. a third of
//     a column of W_hh^T, in 128 registers (loaded once, coalesced along k) and sums its third against the LDS broadcast of dgh in
//     four chains; the three thirds meet in LDS (1.5 KiB) and are added in a fixed order: d h_prev = dh' z + ((p0 + p1) + p2).
// Three barriers per step, no scratch, 3 KiB of LDS; fp32 throughout, no atomics: the same bits on every call.
struct GruBwdP {
    const float* dwords; const float* dsent; const float* gates; const float* hn; const float* hprev;
    const float* w_hh[2];
    float* dgi; float* dgh;
    int B, Tmax;
    int lens[GR_BMAX];
};

__global__ __launch_bounds__(GR_G) void gru_encoder_bwd_kernel(const GruBwdP p) {
    __shared__ __attribute__((aligned(16))) float dGs[GR_G];
    __shared__ float part[3][GR_H];
    const int tid = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int len = min(max(p.lens[b], 0), p.Tmax);
    const int k = tid & (GR_H - 1), qd = tid >> 7;
    float wt[GR_H];
    {
        const float* w = p.w_hh[dir] + (size_t)qd * GR_H * GR_H + k;
#pragma unroll
        for (int jj = 0; jj < GR_H; ++jj) wt[jj] = w[(size_t)jj * GR_H];
    }
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;
    float dh_rec = 0.f;
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir ? len - 1 - s : s;
        float dh_z = 0.f;
        if (tid < GR_H) {
            const int j = tid;
            float dh = dh_rec;
            if (p.dwords) dh += p.dwords[((size_t)b * 2 * GR_H + (size_t)dir * GR_H + j) * p.Tmax + t];
            if (s == len - 1 && p.dsent) dh += p.dsent[(size_t)b * 2 * GR_H + dir * GR_H + j];
            const float* gr = p.gates + (base + t) * GR_G;
            const float r = gr[j], z = gr[GR_H + j], n = gr[2 * GR_H + j];
            const float hn = p.hn[(base + t) * GR_H + j], hp = p.hprev[(base + t) * GR_H + j];
            const float a_n = dh * (1.f - z) * (1.f - n * n);
            const float a_z = dh * (hp - n) * (z * (1.f - z));
            const float a_r = a_n * hn * (r * (1.f - r));
            const float a_nh = a_n * r;
            dh_z = dh * z;
            dGs[j] = a_r; dGs[GR_H + j] = a_z; dGs[2 * GR_H + j] = a_nh;
            float* oi = p.dgi + (base + t) * GR_G;
            float* oh = p.dgh + (base + t) * GR_G;
            oi[j] = a_r; oi[GR_H + j] = a_z; oi[2 * GR_H + j] = a_n;
            oh[j] = a_r; oh[GR_H + j] = a_z; oh[2 * GR_H + j] = a_nh;
        }
        __syncthreads();
        if (s > 0) {                                             // (the same for the whole block)
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            const float* gq = dGs + qd * GR_H;
#pragma unroll
            for (int j4 = 0; j4 < GR_H / 4; ++j4) {
                const float4 gv = *(const float4*)&gq[4 * j4];
                a0 = fmaf(wt[4 * j4], gv.x, a0); a1 = fmaf(wt[4 * j4 + 1], gv.y, a1);
                a2 = fmaf(wt[4 * j4 + 2], gv.z, a2); a3 = fmaf(wt[4 * j4 + 3], gv.w, a3);
            }
            part[qd][k] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        if (s > 0 && tid < GR_H) dh_rec = dh_z + ((part[0][tid] + part[1][tid]) + part[2][tid]);
    }
    for (int t = len; t < p.Tmax; ++t) {
        p.dgi[(base + t) * GR_G + tid] = 0.f;
        p.dgh[(base + t) * GR_G + tid] = 0.f;
    }
}

// dbias[d][row] = sum over the B * Tmax positions of dg[d][.][row], in index order (one thread per (d, row): coalesced rows);
// blockIdx.y picks (dgi -> d b_ih) or (dgh -> d b_hh): the n block of the latter carries the factor r.
__global__ __launch_bounds__(256) void gru_bias_grad_kernel(const float* __restrict__ dgi, const float* __restrict__ dgh, int n,
                                                            float* __restrict__ db_ih, float* __restrict__ db_hh) {
    const float* dg = blockIdx.y ? dgh : dgi;
    float* dbias = blockIdx.y ? db_hh : db_ih;
    if (!dbias) return;                                          // (the same for the whole block)
    const int idx = blockIdx.x * 256 + threadIdx.x;              // < 2 * GR_G
    const int d = idx / GR_G, row = idx - d * GR_G;
    const float* src = dg + (size_t)d * n * GR_G + row;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        a0 += src[(size_t)i * GR_G]; a1 += src[(size_t)(i + 1) * GR_G]; a2 += src[(size_t)(i + 2) * GR_G]; a3 += src[(size_t)(i + 3) * GR_G];
    }
    for (; i < n; ++i) a0 += src[(size_t)i * GR_G];
    dbias[idx] = (a0 + a1) + (a2 + a3);
}

// the checks of both forward entries; fills p (everything but the training fields)
int gru_fill(GruP& p, const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
             const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0, float* words, float* sent,
             int B, int T, int Tmax, int V, int E, int H) {
    if (!captions || !lens_host || !emb || !w_ih || !w_hh || !b_ih || !b_hh || !words || !sent) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > GR_BMAX || H != GR_H || T <= 0 || Tmax <= 0 || Tmax > T || Tmax > GR_TMAX || E <= 0 || E > GR_EMAX || (E % 4) || V <= 0)
        return MOGAN_ERR_SHAPE;
    p.cap = captions; p.emb = emb; p.h0 = h0; p.words = words; p.sent = sent;
    p.B = B; p.T = T; p.Tmax = Tmax; p.V = V; p.E = E;
    p.scale = 1.f;
    for (int d = 0; d < 2; ++d) {
        if (!w_ih[d] || !w_hh[d] || !b_ih[d] || !b_hh[d] || (((uintptr_t)w_ih[d] | (uintptr_t)w_hh[d]) & 15)) return MOGAN_ERR_SHAPE;
        p.w_ih[d] = w_ih[d]; p.w_hh[d] = w_hh[d]; p.b_ih[d] = b_ih[d]; p.b_hh[d] = b_hh[d];
    }
    for (int i = 0; i < B; ++i) { if (lens_host[i] < 0 || lens_host[i] > Tmax) return MOGAN_ERR_SHAPE; p.lens[i] = lens_host[i]; }
    return 0;
}

}  // namespace

extern "C" {

int mogan_gru_encoder_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                          const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                          float* words, float* sent, int B, int T, int Tmax, int V, int E, int H, hipStream_t stream) {
    GruP p{};
    if (int rc = gru_fill(p, captions, lens_host, emb, w_ih, w_hh, b_ih, b_hh, h0, words, sent, B, T, Tmax, V, E, H)) return rc;
    hipLaunchKernelGGL(gru_encoder_kernel<false>, dim3(2 * B), dim3(GR_G), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_gru_encoder_train_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                                const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                                const uint8_t* keep_mask, float scale, float* words, float* sent, float* x, float* gates, float* hn,
                                float* hprev, int B, int T, int Tmax, int V, int E, int H, hipStream_t stream) {
    if (!x || !gates || !hn || !hprev) return MOGAN_ERR_SHAPE;
    GruP p{};
    if (int rc = gru_fill(p, captions, lens_host, emb, w_ih, w_hh, b_ih, b_hh, h0, words, sent, B, T, Tmax, V, E, H)) return rc;
    p.mask = keep_mask; p.scale = scale; p.x = x; p.gates = gates; p.hn = hn; p.hprev = hprev;
    hipLaunchKernelGGL(gru_encoder_kernel<true>, dim3(2 * B), dim3(GR_G), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_gru_encoder_bwd(const float* dwords, const float* dsent, const int* lens_host, const float* gates, const float* hn,
                          const float* hprev, const float* const* w_hh, float* dgi, float* dgh, float* dbias_ih, float* dbias_hh,
                          int B, int Tmax, int H, hipStream_t stream) {
    if (!lens_host || !gates || !hn || !hprev || !w_hh || !dgi || !dgh || !w_hh[0] || !w_hh[1]) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > GR_BMAX || H != GR_H || Tmax <= 0 || Tmax > GR_TMAX) return MOGAN_ERR_SHAPE;
    GruBwdP p{};
    p.dwords = dwords; p.dsent = dsent; p.gates = gates; p.hn = hn; p.hprev = hprev;
    p.w_hh[0] = w_hh[0]; p.w_hh[1] = w_hh[1]; p.dgi = dgi; p.dgh = dgh; p.B = B; p.Tmax = Tmax;
    for (int i = 0; i < B; ++i) { if (lens_host[i] < 0 || lens_host[i] > Tmax) return MOGAN_ERR_SHAPE; p.lens[i] = lens_host[i]; }
    hipLaunchKernelGGL(gru_encoder_bwd_kernel, dim3(2 * B), dim3(GR_G), 0, stream, p);
    if (dbias_ih || dbias_hh)
        hipLaunchKernelGGL(gru_bias_grad_kernel, dim3(2 * GR_G / 256, 2), dim3(256), 0, stream, (const float*)dgi, (const float*)dgh,
                           B * Tmax, dbias_ih, dbias_hh);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

}  // extern "C"
