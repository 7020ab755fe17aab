// mogan_lstm.hip -- the text encoder's recurrent part: the eval forward as ONE launch, and (further down) the training forward,
// back-propagation through time and the embedding gradient of DAMSM pre-training.
//
// RNN_ENCODER (code/coco/attngan/model.py:120-204) embeds the captions (nn.Embedding(n_words, 300)) and runs a one-layer bidirectional
// LSTM (128 units per direction) over the packed sequences; words_emb = the outputs (B, 256, T_max), zero behind every caption's
// end, sent_emb = the two final hidden states (B, 256).  It runs once per train step, frozen, without gradients: 0.1 % of the step's
// FLOPs -- and, on the stock nn.LSTM (MIOpen), 119 launches, 0.37 ms of kernel time and 0.8 ms of host time per step (B = 16, T = 12:
// one GEMM + one update kernel per time step and direction, pack / unpack copies; tools/time_text.py).  Here a block owns one
// (direction, caption):
//   * 512 threads = the 512 gate rows (i, f, g, o x 128 units).  The embedded caption sits in LDS; thread j streams row j of W_ih ONCE
//     and forms its input projection for every time step in registers (bias b_ih + b_hh folded in), parks it in LDS [t][512],
//   * then holds row j of W_hh (128 values) in registers for the recurrence: per step 128 fmas against the hidden state in LDS
//     (broadcast reads), the pre-activations through LDS to the 128 unit threads, which apply the gates (PyTorch's order i, f, g, o:
//     c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c')), write h into the output row of step t and back to LDS; two barriers per step.
// The backward direction walks t = len - 1 ... 0; positions t >= len of words_emb are written as zeros (pad_packed_sequence).
// fp32 throughout; the summation order differs from MIOpen's GEMMs (results agree to ~1e-6 relative, tests/test_kernels_gpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"
#include "mogan_internal.h"

namespace {

constexpr int LS_H = 128, LS_G = 4 * LS_H, LS_TMAX = 32, LS_EMAX = 320, LS_BMAX = 64;

struct LstmP {
    const long long* cap; const float* emb;
    const float* w_ih[2]; const float* w_hh[2]; const float* b_ih[2]; const float* b_hh[2];
    const float* h0; const float* c0;
    float* words; float* sent;
    int B, T, Tmax, V, E;
    int lens[LS_BMAX];
};

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(LS_G) void lstm_encoder_kernel(const LstmP p) {
    __shared__ __attribute__((aligned(16))) float Xs[LS_TMAX * LS_EMAX];      // the embedded caption [t][E]; later: the projections
    __shared__ __attribute__((aligned(16))) float XP[LS_TMAX * LS_G];         // input projections [t][gate row]
    __shared__ __attribute__((aligned(16))) float Hs[LS_H];
    __shared__ float Gs[LS_G];
    const int j = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int E = p.E, len = min(max(p.lens[b], 0), p.Tmax);
    // ---- the caption's embedding rows
    for (int t = 0; t < len; ++t) {
        long long tok = p.cap[(size_t)b * p.T + t];
        tok = tok < 0 ? 0 : (tok >= p.V ? p.V - 1 : tok);
        const float* row = p.emb + (size_t)tok * E;
        if (j < E) Xs[t * LS_EMAX + j] = row[j];
    }
    __syncthreads();
    // ---- input projection of every step: one pass over row j of W_ih
    {
        float acc[LS_TMAX];
        const float bias = p.b_ih[dir][j] + p.b_hh[dir][j];
#pragma unroll
        for (int t = 0; t < LS_TMAX; ++t) acc[t] = bias;
        const float4* wr = (const float4*)(p.w_ih[dir] + (size_t)j * E);
        for (int k4 = 0; k4 < E / 4; ++k4) {
            const float4 w = wr[k4];
#pragma unroll
            for (int t = 0; t < LS_TMAX; ++t)
                if (t < len) {                                   // (the same for the whole block)
                    const float4 x = *(const float4*)&Xs[t * LS_EMAX + 4 * k4];
                    acc[t] = fmaf(w.x, x.x, acc[t]); acc[t] = fmaf(w.y, x.y, acc[t]);
                    acc[t] = fmaf(w.z, x.z, acc[t]); acc[t] = fmaf(w.w, x.w, acc[t]);
                }
        }
#pragma unroll
        for (int t = 0; t < LS_TMAX; ++t) if (t < len) XP[t * LS_G + j] = acc[t];
    }
    // ---- recurrence
    float4 whh[LS_H / 4];
    {
        const float4* hr = (const float4*)(p.w_hh[dir] + (size_t)j * LS_H);
#pragma unroll
        for (int k4 = 0; k4 < LS_H / 4; ++k4) whh[k4] = hr[k4];
    }
    float c = 0.f, h = 0.f;
    if (j < LS_H) {
        const size_t s0 = ((size_t)dir * p.B + b) * LS_H + j;
        if (p.h0) h = p.h0[s0];
        if (p.c0) c = p.c0[s0];
        Hs[j] = h;
    }
    __syncthreads();
    float* wout = p.words + ((size_t)b * 2 * LS_H + (size_t)dir * LS_H) * p.Tmax;
    for (int s = 0; s < len; ++s) {
        const int t = dir ? len - 1 - s : s;
        float a0 = XP[t * LS_G + j], a1 = 0.f, a2 = 0.f, a3 = 0.f;       // four chains, summed at the end
#pragma unroll
        for (int k4 = 0; k4 < LS_H / 4; ++k4) {
            const float4 hv = *(const float4*)&Hs[4 * k4];
            a0 = fmaf(whh[k4].x, hv.x, a0); a1 = fmaf(whh[k4].y, hv.y, a1);
            a2 = fmaf(whh[k4].z, hv.z, a2); a3 = fmaf(whh[k4].w, hv.w, a3);
        }
        Gs[j] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (j < LS_H) {
            const float gi = sigm(Gs[j]), gf = sigm(Gs[LS_H + j]), gg = tanhf(Gs[2 * LS_H + j]), go = sigm(Gs[3 * LS_H + j]);
            c = gf * c + gi * gg;
            h = go * tanhf(c);
            Hs[j] = h;
            wout[(size_t)j * p.Tmax + t] = h;
        }
        __syncthreads();
    }
    if (j < LS_H) {
        p.sent[(size_t)b * 2 * LS_H + dir * LS_H + j] = h;
        for (int t = len; t < p.Tmax; ++t) wout[(size_t)j * p.Tmax + t] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ training (DAMSM pre-training)
// lstm_encoder_train_kernel: the kernel above with embedding dropout (keep mask drawn by the host, row * scale or * 0) and the
// tensors back-propagation needs written on the way: x (the masked, scaled rows), the post-activation gates, c_t, and the hidden
// state that entered each step.  Same thread layout, registers and LDS (~108 KiB); gates through expf / tanhf (no fast-math forms).
struct LstmTrainP {
    LstmP f;
    const uint8_t* mask; float scale;
    float* x; float* gates; float* cells; float* hprev;
};

__global__ __launch_bounds__(LS_G) void lstm_encoder_train_kernel(const LstmTrainP q) {
    __shared__ __attribute__((aligned(16))) float Xs[LS_TMAX * LS_EMAX];
    __shared__ __attribute__((aligned(16))) float XP[LS_TMAX * LS_G];
    __shared__ __attribute__((aligned(16))) float Hs[LS_H];
    __shared__ float Gs[LS_G];
    const LstmP& p = q.f;
    const int j = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int E = p.E, len = min(max(p.lens[b], 0), p.Tmax);
    for (int t = 0; t < p.Tmax; ++t) {
        if (j >= E) break;
        float v = 0.f;
        if (t < len) {
            long long tok = p.cap[(size_t)b * p.T + t];
            tok = tok < 0 ? 0 : (tok >= p.V ? p.V - 1 : tok);
            const float keep = q.mask ? (q.mask[((size_t)b * p.T + t) * E + j] ? q.scale : 0.f) : q.scale;
            v = p.emb[(size_t)tok * E + j] * keep;
            Xs[t * LS_EMAX + j] = v;
        }
        if (dir == 0) q.x[((size_t)b * p.Tmax + t) * E + j] = v;
    }
    __syncthreads();
    {
        float acc[LS_TMAX];
        const float bias = p.b_ih[dir][j] + p.b_hh[dir][j];
#pragma unroll
        for (int t = 0; t < LS_TMAX; ++t) acc[t] = bias;
        const float4* wr = (const float4*)(p.w_ih[dir] + (size_t)j * E);
        for (int k4 = 0; k4 < E / 4; ++k4) {
            const float4 w = wr[k4];
#pragma unroll
            for (int t = 0; t < LS_TMAX; ++t)
                if (t < len) {
                    const float4 x = *(const float4*)&Xs[t * LS_EMAX + 4 * k4];
                    acc[t] = fmaf(w.x, x.x, acc[t]); acc[t] = fmaf(w.y, x.y, acc[t]);
                    acc[t] = fmaf(w.z, x.z, acc[t]); acc[t] = fmaf(w.w, x.w, acc[t]);
                }
        }
#pragma unroll
        for (int t = 0; t < LS_TMAX; ++t) if (t < len) XP[t * LS_G + j] = acc[t];
    }
    float4 whh[LS_H / 4];
    {
        const float4* hr = (const float4*)(p.w_hh[dir] + (size_t)j * LS_H);
#pragma unroll
        for (int k4 = 0; k4 < LS_H / 4; ++k4) whh[k4] = hr[k4];
    }
    float c = 0.f, h = 0.f;
    if (j < LS_H) {
        const size_t s0 = ((size_t)dir * p.B + b) * LS_H + j;
        if (p.h0) h = p.h0[s0];
        if (p.c0) c = p.c0[s0];
        Hs[j] = h;
    }
    __syncthreads();
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;                    // row (dir, b, t = 0) of the saved tensors
    float* wout = p.words + ((size_t)b * 2 * LS_H + (size_t)dir * LS_H) * p.Tmax;
    for (int s = 0; s < len; ++s) {
        const int t = dir ? len - 1 - s : s;
        float a0 = XP[t * LS_G + j], a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < LS_H / 4; ++k4) {
            const float4 hv = *(const float4*)&Hs[4 * k4];
            a0 = fmaf(whh[k4].x, hv.x, a0); a1 = fmaf(whh[k4].y, hv.y, a1);
            a2 = fmaf(whh[k4].z, hv.z, a2); a3 = fmaf(whh[k4].w, hv.w, a3);
        }
        Gs[j] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (j < LS_H) {
            const float gi = sigm(Gs[j]), gf = sigm(Gs[LS_H + j]), gg = tanhf(Gs[2 * LS_H + j]), go = sigm(Gs[3 * LS_H + j]);
            float* gr = q.gates + (base + t) * LS_G;
            gr[j] = gi; gr[LS_H + j] = gf; gr[2 * LS_H + j] = gg; gr[3 * LS_H + j] = go;
            q.hprev[(base + t) * LS_H + j] = h;
            c = gf * c + gi * gg;
            h = go * tanhf(c);
            q.cells[(base + t) * LS_H + j] = c;
            Hs[j] = h;
            wout[(size_t)j * p.Tmax + t] = h;
        }
        __syncthreads();
    }
    if (j < LS_H) {
        p.sent[(size_t)b * 2 * LS_H + dir * LS_H + j] = h;
        for (int t = len; t < p.Tmax; ++t) {
            wout[(size_t)j * p.Tmax + t] = 0.f;
            q.cells[(base + t) * LS_H + j] = 0.f;
            q.hprev[(base + t) * LS_H + j] = 0.f;
        }
    }
    for (int t = len; t < p.Tmax; ++t) q.gates[(base + t) * LS_G + j] = 0.f;
}

// lstm_encoder_bwd_kernel: back-propagation through time, one block of 512 threads per (direction, caption), walking the forward's
// steps backwards.  Per step
//   * the 128 unit threads (tid < 128) turn d h_t (= d words[:, t] + the recurrent part + d sent at the walk's last step) and the
//     running d c into the four pre-activation gate gradients (i, f, g, o), write them to dgates and to LDS (2 KiB),
//   * then all 512 threads form d h_prev = W_hh^T . dG_t: thread (k = tid % 128, q = tid / 128) holds W_hh[q * 128 ... + 127][k],
//     i.e. a quarter column of W_hh^T, in 128 registers (loaded once, coalesced along k) and sums its quarter against the LDS
//     broadcast of dG_t in four chains; the four quarters meet in LDS (2 KiB) and are added in a fixed order.
// Three barriers per step, 176 VGPRs (no scratch), 4 KiB of LDS; fp32 and tanhf throughout, no atomics: the same bits on every call.
struct LstmBwdP {
    const float* dwords; const float* dsent; const float* gates; const float* cells; const float* hprev; const float* c0;
    const float* w_hh[2];
    float* dg;
    int B, Tmax;
    int lens[LS_BMAX];
};

__global__ __launch_bounds__(LS_G) void lstm_encoder_bwd_kernel(const LstmBwdP p) {
    __shared__ __attribute__((aligned(16))) float dGs[LS_G];
    __shared__ float part[4][LS_H];
    const int tid = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int len = min(max(p.lens[b], 0), p.Tmax);
    const int k = tid & (LS_H - 1), qd = tid >> 7;
    float wt[LS_H];
    {
        const float* w = p.w_hh[dir] + (size_t)qd * LS_H * LS_H + k;
#pragma unroll
        for (int jj = 0; jj < LS_H; ++jj) wt[jj] = w[(size_t)jj * LS_H];
    }
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;
    float dh_rec = 0.f, dc = 0.f;
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir ? len - 1 - s : s;
        if (tid < LS_H) {
            const int j = tid;
            float dh = dh_rec;
            if (p.dwords) dh += p.dwords[((size_t)b * 2 * LS_H + (size_t)dir * LS_H + j) * p.Tmax + t];
            if (s == len - 1 && p.dsent) dh += p.dsent[(size_t)b * 2 * LS_H + dir * LS_H + j];
            const float* gr = p.gates + (base + t) * LS_G;
            const float gi = gr[j], gf = gr[LS_H + j], gg = gr[2 * LS_H + j], go = gr[3 * LS_H + j];
            const float c = p.cells[(base + t) * LS_H + j];
            float cp;
            if (s > 0) cp = p.cells[(base + (dir ? t + 1 : t - 1)) * LS_H + j];
            else cp = p.c0 ? p.c0[((size_t)dir * p.B + b) * LS_H + j] : 0.f;
            const float tc = tanhf(c);
            const float d_o = dh * tc;
            const float dcc = dc + dh * go * (1.f - tc * tc);
            const float a_i = dcc * gg * (gi * (1.f - gi));
            const float a_f = dcc * cp * (gf * (1.f - gf));
            const float a_g = dcc * gi * (1.f - gg * gg);
            const float a_o = d_o * (go * (1.f - go));
            dc = dcc * gf;
            dGs[j] = a_i; dGs[LS_H + j] = a_f; dGs[2 * LS_H + j] = a_g; dGs[3 * LS_H + j] = a_o;
            float* o = p.dg + (base + t) * LS_G;
            o[j] = a_i; o[LS_H + j] = a_f; o[2 * LS_H + j] = a_g; o[3 * LS_H + j] = a_o;
        }
        __syncthreads();
        if (s > 0) {                                             // (the same for the whole block)
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            const float* gq = dGs + qd * LS_H;
#pragma unroll
            for (int j4 = 0; j4 < LS_H / 4; ++j4) {
                const float4 gv = *(const float4*)&gq[4 * j4];
                a0 = fmaf(wt[4 * j4], gv.x, a0); a1 = fmaf(wt[4 * j4 + 1], gv.y, a1);
                a2 = fmaf(wt[4 * j4 + 2], gv.z, a2); a3 = fmaf(wt[4 * j4 + 3], gv.w, a3);
            }
            part[qd][k] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        if (s > 0 && tid < LS_H) dh_rec = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    }
    for (int t = len; t < p.Tmax; ++t) p.dg[(base + t) * LS_G + tid] = 0.f;
}

// dbias[d][row] = sum over the B * Tmax positions of dgates[d][.][row], in index order (one thread per (d, row): coalesced rows)
__global__ __launch_bounds__(256) void lstm_bias_grad_kernel(const float* __restrict__ dg, int n, float* __restrict__ dbias) {
    const int idx = blockIdx.x * 256 + threadIdx.x;              // < 2 * LS_G
    const int d = idx / LS_G, row = idx - d * LS_G;
    const float* src = dg + (size_t)d * n * LS_G + row;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        a0 += src[(size_t)i * LS_G]; a1 += src[(size_t)(i + 1) * LS_G]; a2 += src[(size_t)(i + 2) * LS_G]; a3 += src[(size_t)(i + 3) * LS_G];
    }
    for (; i < n; ++i) a0 += src[(size_t)i * LS_G];
    dbias[idx] = (a0 + a1) + (a2 + a3);
}

// embedding_bwd_kernel: one block per position (b, t).  A block whose token already occurs at an earlier valid position leaves; the
// others own their token's row: they add the (masked, scaled) dx rows of every position that holds the token, in index order, and
// add the sum to demb[tok].  B * Tmax <= 2048 positions: the all-pairs token compare is one pass per block.
struct EmbBwdP {
    const long long* cap; const float* dx; const uint8_t* mask; float scale; float* demb;
    int B, T, Tmax, V, E;
    int lens[LS_BMAX];
};

__global__ __launch_bounds__(256) void embedding_bwd_kernel(const EmbBwdP p) {
    __shared__ unsigned char match[LS_BMAX * LS_TMAX];
    __shared__ int lens[LS_BMAX];
    const int tid = threadIdx.x, pos = blockIdx.x, b = pos / p.Tmax, t = pos - b * p.Tmax;
    if (t >= min(max(p.lens[b], 0), p.Tmax)) return;           // (the same for the whole block)
    if (tid < LS_BMAX) lens[tid] = tid < p.B ? min(max(p.lens[tid], 0), p.Tmax) : 0;
    __syncthreads();
    auto token = [&](int qb, int qt) -> long long {
        long long tok = p.cap[(size_t)qb * p.T + qt];
        return tok < 0 ? 0 : (tok >= p.V ? p.V - 1 : tok);
    };
    const long long tok = token(b, t);
    const int N = p.B * p.Tmax;
    int earlier = 0;
    for (int q = tid; q < N; q += 256) {
        const int qb = q / p.Tmax, qt = q - qb * p.Tmax;
        const bool m = qt < lens[qb] && token(qb, qt) == tok;
        match[q] = m ? 1 : 0;
        if (m && q < pos) earlier = 1;
    }
    if (__syncthreads_or(earlier)) return;
    for (int e = tid; e < p.E; e += 256) {
        float acc = 0.f;
        for (int q = pos; q < N; ++q)
            if (match[q]) {
                const int qb = q / p.Tmax, qt = q - qb * p.Tmax;
                const float keep = p.mask ? (p.mask[((size_t)qb * p.T + qt) * p.E + e] ? p.scale : 0.f) : p.scale;
                acc += keep * p.dx[(size_t)q * p.E + e];
            }
        p.demb[(size_t)tok * p.E + e] += acc;
    }
}

}  // namespace

extern "C" {

int mogan_lstm_encoder_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                           const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                           const float* c0, float* words, float* sent, int B, int T, int Tmax, int V, int E, int H,
                           hipStream_t stream) {
    if (!captions || !lens_host || !emb || !w_ih || !w_hh || !b_ih || !b_hh || !words || !sent) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > LS_BMAX || H != LS_H || T <= 0 || Tmax <= 0 || Tmax > T || Tmax > LS_TMAX || E <= 0 || E > LS_EMAX || (E % 4) || V <= 0)
        return MOGAN_ERR_SHAPE;
    LstmP p{};
    p.cap = captions; p.emb = emb; p.h0 = h0; p.c0 = c0; p.words = words; p.sent = sent;
    p.B = B; p.T = T; p.Tmax = Tmax; p.V = V; p.E = E;
    for (int d = 0; d < 2; ++d) {
        if (!w_ih[d] || !w_hh[d] || !b_ih[d] || !b_hh[d] || (((uintptr_t)w_ih[d] | (uintptr_t)w_hh[d]) & 15)) return MOGAN_ERR_SHAPE;
        p.w_ih[d] = w_ih[d]; p.w_hh[d] = w_hh[d]; p.b_ih[d] = b_ih[d]; p.b_hh[d] = b_hh[d];
    }
    for (int i = 0; i < B; ++i) { if (lens_host[i] < 0 || lens_host[i] > Tmax) return MOGAN_ERR_SHAPE; p.lens[i] = lens_host[i]; }
    hipLaunchKernelGGL(lstm_encoder_kernel, dim3(2 * B), dim3(LS_G), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_lstm_encoder_train_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                                 const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                                 const float* c0, const uint8_t* keep_mask, float scale, float* words, float* sent, float* x,
                                 float* gates, float* cells, float* hprev, int B, int T, int Tmax, int V, int E, int H,
                                 hipStream_t stream) {
    if (!captions || !lens_host || !emb || !w_ih || !w_hh || !b_ih || !b_hh || !words || !sent || !x || !gates || !cells || !hprev)
        return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > LS_BMAX || H != LS_H || T <= 0 || Tmax <= 0 || Tmax > T || Tmax > LS_TMAX || E <= 0 || E > LS_EMAX || (E % 4) || V <= 0)
        return MOGAN_ERR_SHAPE;
    LstmTrainP q{};
    LstmP& p = q.f;
    p.cap = captions; p.emb = emb; p.h0 = h0; p.c0 = c0; p.words = words; p.sent = sent;
    p.B = B; p.T = T; p.Tmax = Tmax; p.V = V; p.E = E;
    q.mask = keep_mask; q.scale = scale; q.x = x; q.gates = gates; q.cells = cells; q.hprev = hprev;
    for (int d = 0; d < 2; ++d) {
        if (!w_ih[d] || !w_hh[d] || !b_ih[d] || !b_hh[d] || (((uintptr_t)w_ih[d] | (uintptr_t)w_hh[d]) & 15)) return MOGAN_ERR_SHAPE;
        p.w_ih[d] = w_ih[d]; p.w_hh[d] = w_hh[d]; p.b_ih[d] = b_ih[d]; p.b_hh[d] = b_hh[d];
    }
    for (int i = 0; i < B; ++i) { if (lens_host[i] < 0 || lens_host[i] > Tmax) return MOGAN_ERR_SHAPE; p.lens[i] = lens_host[i]; }
    hipLaunchKernelGGL(lstm_encoder_train_kernel, dim3(2 * B), dim3(LS_G), 0, stream, q);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_lstm_encoder_bwd(const float* dwords, const float* dsent, const int* lens_host, const float* gates, const float* cells,
                           const float* hprev, const float* c0, const float* const* w_hh, float* dgates, float* dbias, int B,
                           int Tmax, int H, hipStream_t stream) {
    if (!lens_host || !gates || !cells || !hprev || !w_hh || !dgates || !w_hh[0] || !w_hh[1]) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > LS_BMAX || H != LS_H || Tmax <= 0 || Tmax > LS_TMAX) return MOGAN_ERR_SHAPE;
    LstmBwdP p{};
    p.dwords = dwords; p.dsent = dsent; p.gates = gates; p.cells = cells; p.hprev = hprev; p.c0 = c0;
    p.w_hh[0] = w_hh[0]; p.w_hh[1] = w_hh[1]; p.dg = dgates; p.B = B; p.Tmax = Tmax;
    for (int i = 0; i < B; ++i) { if (lens_host[i] < 0 || lens_host[i] > Tmax) return MOGAN_ERR_SHAPE; p.lens[i] = lens_host[i]; }
    hipLaunchKernelGGL(lstm_encoder_bwd_kernel, dim3(2 * B), dim3(LS_G), 0, stream, p);
    if (dbias)
        hipLaunchKernelGGL(lstm_bias_grad_kernel, dim3(2 * LS_G / 256), dim3(256), 0, stream, (const float*)dgates, B * Tmax, dbias);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_embedding_bwd(const long long* captions, const int* lens_host, const float* dx, const uint8_t* keep_mask, float scale,
                        float* demb, int B, int T, int Tmax, int V, int E, hipStream_t stream) {
    if (!captions || !lens_host || !dx || !demb) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > LS_BMAX || T <= 0 || Tmax <= 0 || Tmax > T || Tmax > LS_TMAX || E <= 0 || E > LS_EMAX || (E % 4) || V <= 0)
        return MOGAN_ERR_SHAPE;
    EmbBwdP p{};
    p.cap = captions; p.dx = dx; p.mask = keep_mask; p.scale = scale; p.demb = demb;
    p.B = B; p.T = T; p.Tmax = Tmax; p.V = V; p.E = E;
    for (int i = 0; i < B; ++i) { if (lens_host[i] < 0 || lens_host[i] > Tmax) return MOGAN_ERR_SHAPE; p.lens[i] = lens_host[i]; }
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3(B * Tmax), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

}  // extern "C"
