// mogan_rnn.hip -- the text encoder's recurrent part for both cells (cfg.RNN_TYPE = 'LSTM' / 'GRU'): the eval forward as ONE launch,
// the training forward and back-propagation through time of DAMSM pre-training as one launch each, the bias gradients and the
// embedding gradient.  The weight-gradient GEMMs are mogan_bmm's.
//
// RNN_ENCODER (code/coco/attngan/model.py:120-204) embeds the captions (nn.Embedding(n_words, 300)) and runs a one-layer bidirectional
// nn.LSTM or nn.GRU (H = 128 units per direction) over the packed sequences; words_emb = the outputs (B, 256, T_max), zero behind
// every caption's end, sent_emb = the two final hidden states (B, 256).  In the GAN step it runs once, frozen, without gradients:
// 0.1 % of the step's FLOPs -- and, on the stock nn.LSTM (MIOpen), 119 launches, 0.37 ms of kernel time and 0.8 ms of host time per
// step (B = 16, T = 12: one GEMM + one update kernel per time step and direction, pack / unpack copies; tools/time_text.py).
// Here a block owns one (direction, caption) and has one thread per gate row, G = 4 H (LSTM: i, f, g, o) or 3 H (GRU: r, z, n):
//   * the embedded caption sits in LDS (<= 40 KiB); thread j streams row j of W_ih ONCE and forms its input projection for every time
//     step in registers, the bias folded in, and parks it in LDS [t][G] (<= 64 KiB),
//   * then holds row j of W_hh (128 values) in registers for the recurrence: per step 128 fmas against the hidden state in LDS
//     (broadcast reads), the results through LDS to the 128 unit threads, which apply the cell's gates, write h into the output row
//     of step t and back to LDS; two barriers per step.
// The stages are written once (stage_caption ... sum_partials below); the cells' own mathematics sits in the four kernel bodies:
//   LSTM   c' = s(f) c + s(i) tanh(g),  h' = s(o) tanh(c');  b_ih + b_hh folded into every row's projection
//   GRU    r = s(W_ir x + b_ir + W_hr h + b_hr)      z = s(W_iz x + b_iz + W_hz h + b_hz)
//          hn = W_hn h + b_hn                        n = tanh(W_in x + b_in + r * hn)            h' = (1 - z) * n + z * h
//          the r and z rows fold b_ih + b_hh, the n rows b_ih only, because b_hn sits inside r * (...)
// The reverse direction walks t = len - 1 ... 0; positions t >= len of words_emb are written as zeros (pad_packed_sequence).
// fp32 throughout, expf / tanhf (no fast-math forms), no atomics; the summation order differs from MIOpen's GEMMs (results agree
// to ~1e-6 relative, tests/test_kernels_gpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"
#include "mogan_internal.h"

namespace {

constexpr int RN_H = 128, RN_TMAX = 32, RN_EMAX = 320, RN_BMAX = 64;
constexpr int LS_G = 4 * RN_H, GR_G = 3 * RN_H;

// what both cells' forward kernels take; the training fields are NULL / 1 in the eval kernels
struct RnnP {
    const long long* cap; const float* emb;
    const float* w_ih[2]; const float* w_hh[2]; const float* b_ih[2]; const float* b_hh[2];
    const float* h0;
    float* words; float* sent;
    // training only: embedding dropout and what back-propagation needs
    const uint8_t* mask; float scale;
    float* x; float* gates; float* hprev;
    int B, T, Tmax, V, E;
    int lens[RN_BMAX];
};
struct LstmP : RnnP { const float* c0; float* cells; };
struct GruP : RnnP { float* hn; };

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------------------------------------------------ forward stages
// The forward kernels' LDS is one array, the recurrence's small buffers first: their reads then fit the LDS instructions' 16-bit
// immediate offsets (behind the 88 KiB of Xs / XP every one of the 32 reads of Hs per step would need an address register of its
// own: scratch).  Hs [H]: the hidden state; Gs [G]: the step's pre-activations; XP [t][G]: input projections; Xs [t][E]: the caption.
template <int G> constexpr int FWD_LDS = RN_H + G + RN_TMAX * G + RN_TMAX * RN_EMAX;

// the caption's embedding rows into Xs.  TRAIN: row * (keep ? scale : 0), and the forward direction's block writes the rows (zeros
// at t >= len) to x
template <bool TRAIN, class P>                                  // P: LstmP or GruP
__device__ __forceinline__ void stage_caption(const P& p, float* Xs, int j, int dir, int b, int len) {
    const int E = p.E;
    if (j < E) {
        for (int t = 0; t < (TRAIN ? p.Tmax : len); ++t) {
            float v = 0.f;
            if (t < len) {
                long long tok = p.cap[(size_t)b * p.T + t];
                tok = tok < 0 ? 0 : (tok >= p.V ? p.V - 1 : tok);
                v = p.emb[(size_t)tok * E + j];
                if (TRAIN) v *= p.mask ? (p.mask[((size_t)b * p.T + t) * E + j] ? p.scale : 0.f) : p.scale;
                Xs[t * RN_EMAX + j] = v;
            }
            if (TRAIN && dir == 0) p.x[((size_t)b * p.Tmax + t) * E + j] = v;
        }
    }
}

// input projection of every step: one pass over row j of W_ih, XP[t][j] = bias + W_ih[j] . Xs[t]
template <int G>
__device__ __forceinline__ void input_projection(const float* w_ih_row, float bias, const float* Xs, float* XP, int j, int E, int len) {
    float acc[RN_TMAX];
#pragma unroll
    for (int t = 0; t < RN_TMAX; ++t) acc[t] = bias;
    const float4* wr = (const float4*)w_ih_row;
    for (int k4 = 0; k4 < E / 4; ++k4) {
        const float4 w = wr[k4];
#pragma unroll
        for (int t = 0; t < RN_TMAX; ++t)
            if (t < len) {                                       // (the same for the whole block)
                const float4 x = *(const float4*)&Xs[t * RN_EMAX + 4 * k4];
                acc[t] = fmaf(w.x, x.x, acc[t]); acc[t] = fmaf(w.y, x.y, acc[t]);
                acc[t] = fmaf(w.z, x.z, acc[t]); acc[t] = fmaf(w.w, x.w, acc[t]);
            }
    }
#pragma unroll
    for (int t = 0; t < RN_TMAX; ++t) if (t < len) XP[t * G + j] = acc[t];
}

__device__ __forceinline__ void load_whh_row(float4 (&whh)[RN_H / 4], const float* w_hh_row) {
    const float4* hr = (const float4*)w_hh_row;
#pragma unroll
    for (int k4 = 0; k4 < RN_H / 4; ++k4) whh[k4] = hr[k4];
}

// a0 + W_hh[j] . Hs: four chains, summed at the end
__device__ __forceinline__ float dot_hidden(const float4 (&whh)[RN_H / 4], const float* Hs, float a0) {
    float a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < RN_H / 4; ++k4) {
        const float4 hv = *(const float4*)&Hs[4 * k4];
        a0 = fmaf(whh[k4].x, hv.x, a0); a1 = fmaf(whh[k4].y, hv.y, a1);
        a2 = fmaf(whh[k4].z, hv.z, a2); a3 = fmaf(whh[k4].w, hv.w, a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// ------------------------------------------------------------------------------------------------ forward kernels
// TRAIN = false: the eval forward.  TRAIN = true: the same arithmetic with embedding dropout (keep mask drawn by the host) and the
// tensors back-propagation needs written on the way: x (the masked, scaled rows), the post-activation gates, the hidden state that
// entered each step, and c_t (LSTM) or hn (GRU); all zero at t >= len.
template <bool TRAIN>
__global__ __launch_bounds__(LS_G) void lstm_encoder_kernel(const LstmP p) {
    __shared__ __attribute__((aligned(16))) float smem[FWD_LDS<LS_G>];
    float* const Hs = smem;
    float* const Gs = Hs + RN_H;
    float* const XP = Gs + LS_G;
    float* const Xs = XP + RN_TMAX * LS_G;
    const int j = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int E = p.E, len = min(max(p.lens[b], 0), p.Tmax);
    stage_caption<TRAIN>(p, Xs, j, dir, b, len);
    __syncthreads();
    input_projection<LS_G>(p.w_ih[dir] + (size_t)j * E, p.b_ih[dir][j] + p.b_hh[dir][j], Xs, XP, j, E, len);
    float4 whh[RN_H / 4];
    load_whh_row(whh, p.w_hh[dir] + (size_t)j * RN_H);
    float c = 0.f, h = 0.f;
    if (j < RN_H) {
        const size_t s0 = ((size_t)dir * p.B + b) * RN_H + j;
        if (p.h0) h = p.h0[s0];
        if (p.c0) c = p.c0[s0];
        Hs[j] = h;
    }
    __syncthreads();
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;                    // row (dir, b, t = 0) of the saved tensors
    float* wout = p.words + ((size_t)b * 2 * RN_H + (size_t)dir * RN_H) * p.Tmax;
    for (int s = 0; s < len; ++s) {
        const int t = dir ? len - 1 - s : s;
        Gs[j] = dot_hidden(whh, Hs, XP[t * LS_G + j]);
        __syncthreads();
        if (j < RN_H) {
            const float gi = sigm(Gs[j]), gf = sigm(Gs[RN_H + j]), gg = tanhf(Gs[2 * RN_H + j]), go = sigm(Gs[3 * RN_H + j]);
            if (TRAIN) {
                float* gr = p.gates + (base + t) * LS_G;
                gr[j] = gi; gr[RN_H + j] = gf; gr[2 * RN_H + j] = gg; gr[3 * RN_H + j] = go;
                p.hprev[(base + t) * RN_H + j] = h;
            }
            c = gf * c + gi * gg;
            h = go * tanhf(c);
            if (TRAIN) p.cells[(base + t) * RN_H + j] = c;
            Hs[j] = h;
            wout[(size_t)j * p.Tmax + t] = h;
        }
        __syncthreads();
    }
    if (j < RN_H) {
        p.sent[(size_t)b * 2 * RN_H + dir * RN_H + j] = h;
        for (int t = len; t < p.Tmax; ++t) {
            wout[(size_t)j * p.Tmax + t] = 0.f;
            if (TRAIN) { p.cells[(base + t) * RN_H + j] = 0.f; p.hprev[(base + t) * RN_H + j] = 0.f; }
        }
    }
    if (TRAIN)
        for (int t = len; t < p.Tmax; ++t) p.gates[(base + t) * LS_G + j] = 0.f;
}

template <bool TRAIN>
__global__ __launch_bounds__(GR_G) void gru_encoder_kernel(const GruP p) {
    __shared__ __attribute__((aligned(16))) float smem[FWD_LDS<GR_G>];
    float* const Hs = smem;
    float* const Gs = Hs + RN_H;                                 // r, z pre-activations and hn of the step
    float* const XP = Gs + GR_G;
    float* const Xs = XP + RN_TMAX * GR_G;
    const int j = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int E = p.E, len = min(max(p.lens[b], 0), p.Tmax);
    stage_caption<TRAIN>(p, Xs, j, dir, b, len);
    __syncthreads();
    const float bhh = p.b_hh[dir][j];
    const bool nrow = j >= 2 * RN_H;                             // (the same for a whole wave)
    input_projection<GR_G>(p.w_ih[dir] + (size_t)j * E, p.b_ih[dir][j] + (nrow ? 0.f : bhh), Xs, XP, j, E, len);
    float4 whh[RN_H / 4];
    load_whh_row(whh, p.w_hh[dir] + (size_t)j * RN_H);
    float h = 0.f;
    if (j < RN_H) {
        if (p.h0) h = p.h0[((size_t)dir * p.B + b) * RN_H + j];
        Hs[j] = h;
    }
    __syncthreads();
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;                    // row (dir, b, t = 0) of the saved tensors
    float* wout = p.words + ((size_t)b * 2 * RN_H + (size_t)dir * RN_H) * p.Tmax;
    for (int s = 0; s < len; ++s) {
        const int t = dir ? len - 1 - s : s;
        Gs[j] = dot_hidden(whh, Hs, nrow ? bhh : XP[t * GR_G + j]);          // r, z: the pre-activation; n rows: hn
        __syncthreads();
        if (j < RN_H) {
            const float r = sigm(Gs[j]), z = sigm(Gs[RN_H + j]), hn = Gs[2 * RN_H + j];
            const float n = tanhf(XP[t * GR_G + 2 * RN_H + j] + r * hn);
            if (TRAIN) {
                float* gr = p.gates + (base + t) * GR_G;
                gr[j] = r; gr[RN_H + j] = z; gr[2 * RN_H + j] = n;
                p.hn[(base + t) * RN_H + j] = hn;
                p.hprev[(base + t) * RN_H + j] = h;
            }
            h = (1.f - z) * n + z * h;
            Hs[j] = h;
            wout[(size_t)j * p.Tmax + t] = h;
        }
        __syncthreads();
    }
    if (j < RN_H) {
        p.sent[(size_t)b * 2 * RN_H + dir * RN_H + j] = h;
        for (int t = len; t < p.Tmax; ++t) {
            wout[(size_t)j * p.Tmax + t] = 0.f;
            if (TRAIN) { p.hn[(base + t) * RN_H + j] = 0.f; p.hprev[(base + t) * RN_H + j] = 0.f; }
        }
    }
    if (TRAIN)
        for (int t = len; t < p.Tmax; ++t) p.gates[(base + t) * GR_G + j] = 0.f;
}

// ------------------------------------------------------------------------------------------------ backward stages
// Back-propagation through time: one block of G threads per (direction, caption), walking the forward's steps backwards.  Per step
//   * the 128 unit threads (tid < 128) turn d h_t (= d words[:, t] + the recurrent part + d sent at the walk's last step) into the
//     pre-activation gate gradients, write them out and to LDS (dGs, G floats),
//   * then all G threads form W_hh^T . dGs: thread (k = tid % 128, q = tid / 128) holds W_hh[q * 128 ... + 127][k], i.e. a G / H-th
//     of a column of W_hh^T, in 128 registers (loaded once, coalesced along k) and sums its part against the LDS broadcast of dGs
//     in four chains; the G / H parts meet in LDS (part, G floats) and are added in a fixed order.
// Three barriers per step, no scratch; fp32 and tanhf throughout, no atomics: the same bits on every call.
struct RnnBwdP {
    const float* dwords; const float* dsent; const float* gates; const float* hprev;
    const float* w_hh[2];
    int B, Tmax;
    int lens[RN_BMAX];
};
struct LstmBwdP : RnnBwdP { const float* cells; const float* c0; float* dg; };
struct GruBwdP : RnnBwdP { const float* hn; float* dgi; float* dgh; };

// wt[jj] = W_hh[q * 128 + jj][k]; w_hh_t points at W_hh[q * 128][k]
__device__ __forceinline__ void load_whh_transposed(float (&wt)[RN_H], const float* w_hh_t) {
#pragma unroll
    for (int jj = 0; jj < RN_H; ++jj) wt[jj] = w_hh_t[(size_t)jj * RN_H];
}

__device__ __forceinline__ float dot_gate_grads(const float (&wt)[RN_H], const float* gq) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int j4 = 0; j4 < RN_H / 4; ++j4) {
        const float4 gv = *(const float4*)&gq[4 * j4];
        a0 = fmaf(wt[4 * j4], gv.x, a0); a1 = fmaf(wt[4 * j4 + 1], gv.y, a1);
        a2 = fmaf(wt[4 * j4 + 2], gv.z, a2); a3 = fmaf(wt[4 * j4 + 3], gv.w, a3);
    }
    return (a0 + a1) + (a2 + a3);
}

template <int G>
__device__ __forceinline__ float sum_partials(const float (*part)[RN_H], int k) {
    static_assert(G == 3 * RN_H || G == 4 * RN_H, "three or four gate rows per unit");
    if (G == 4 * RN_H) return (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
    return (part[0][k] + part[1][k]) + part[2][k];
}

// ------------------------------------------------------------------------------------------------ backward kernels
// LSTM: the unit threads carry the running d c and form the four gate gradients (i, f, g, o); d h_prev = the sum of the partials.
__global__ __launch_bounds__(LS_G) void lstm_encoder_bwd_kernel(const LstmBwdP p) {
    __shared__ __attribute__((aligned(16))) float dGs[LS_G];
    __shared__ float part[LS_G / RN_H][RN_H];
    const int tid = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int len = min(max(p.lens[b], 0), p.Tmax);
    const int k = tid & (RN_H - 1), qd = tid >> 7;
    float wt[RN_H];
    load_whh_transposed(wt, p.w_hh[dir] + (size_t)qd * RN_H * RN_H + k);
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;
    float dh_rec = 0.f, dc = 0.f;
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir ? len - 1 - s : s;
        if (tid < RN_H) {
            const int j = tid;
            float dh = dh_rec;
            if (p.dwords) dh += p.dwords[((size_t)b * 2 * RN_H + (size_t)dir * RN_H + j) * p.Tmax + t];
            if (s == len - 1 && p.dsent) dh += p.dsent[(size_t)b * 2 * RN_H + dir * RN_H + j];
            const float* gr = p.gates + (base + t) * LS_G;
            const float gi = gr[j], gf = gr[RN_H + j], gg = gr[2 * RN_H + j], go = gr[3 * RN_H + j];
            const float c = p.cells[(base + t) * RN_H + j];
            float cp;
            if (s > 0) cp = p.cells[(base + (dir ? t + 1 : t - 1)) * RN_H + j];
            else cp = p.c0 ? p.c0[((size_t)dir * p.B + b) * RN_H + j] : 0.f;
            const float tc = tanhf(c);
            const float d_o = dh * tc;
            const float dcc = dc + dh * go * (1.f - tc * tc);
            const float a_i = dcc * gg * (gi * (1.f - gi));
            const float a_f = dcc * cp * (gf * (1.f - gf));
            const float a_g = dcc * gi * (1.f - gg * gg);
            const float a_o = d_o * (go * (1.f - go));
            dc = dcc * gf;
            dGs[j] = a_i; dGs[RN_H + j] = a_f; dGs[2 * RN_H + j] = a_g; dGs[3 * RN_H + j] = a_o;
            float* o = p.dg + (base + t) * LS_G;
            o[j] = a_i; o[RN_H + j] = a_f; o[2 * RN_H + j] = a_g; o[3 * RN_H + j] = a_o;
        }
        __syncthreads();
        if (s > 0) part[qd][k] = dot_gate_grads(wt, dGs + qd * RN_H);        // (the same for the whole block)
        __syncthreads();
        if (s > 0 && tid < RN_H) dh_rec = sum_partials<LS_G>(part, tid);
    }
    for (int t = len; t < p.Tmax; ++t) p.dg[(base + t) * LS_G + tid] = 0.f;
}

// GRU: dn = dh' (1 - z)(1 - n^2),  dz = dh' (h_prev - n) z (1 - z),  dr = dn hn r (1 - r).  The input-side gradients are
// dgi = (dr, dz, dn), the hidden-side ones dgh = (dr, dz, dn r) (b_hn and W_hn sit inside r * (...)); dgh goes through LDS, and
// d h_prev = dh' z + the sum of the partials.
__global__ __launch_bounds__(GR_G) void gru_encoder_bwd_kernel(const GruBwdP p) {
    __shared__ __attribute__((aligned(16))) float dGs[GR_G];
    __shared__ float part[GR_G / RN_H][RN_H];
    const int tid = threadIdx.x, dir = blockIdx.x & 1, b = blockIdx.x >> 1;
    const int len = min(max(p.lens[b], 0), p.Tmax);
    const int k = tid & (RN_H - 1), qd = tid >> 7;
    float wt[RN_H];
    load_whh_transposed(wt, p.w_hh[dir] + (size_t)qd * RN_H * RN_H + k);
    const size_t base = ((size_t)dir * p.B + b) * p.Tmax;
    float dh_rec = 0.f;
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir ? len - 1 - s : s;
        float dh_z = 0.f;
        if (tid < RN_H) {
            const int j = tid;
            float dh = dh_rec;
            if (p.dwords) dh += p.dwords[((size_t)b * 2 * RN_H + (size_t)dir * RN_H + j) * p.Tmax + t];
            if (s == len - 1 && p.dsent) dh += p.dsent[(size_t)b * 2 * RN_H + dir * RN_H + j];
            const float* gr = p.gates + (base + t) * GR_G;
            const float r = gr[j], z = gr[RN_H + j], n = gr[2 * RN_H + j];
            const float hn = p.hn[(base + t) * RN_H + j], hp = p.hprev[(base + t) * RN_H + j];
            const float a_n = dh * (1.f - z) * (1.f - n * n);
            const float a_z = dh * (hp - n) * (z * (1.f - z));
            const float a_r = a_n * hn * (r * (1.f - r));
            const float a_nh = a_n * r;
            dh_z = dh * z;
            dGs[j] = a_r; dGs[RN_H + j] = a_z; dGs[2 * RN_H + j] = a_nh;
            float* oi = p.dgi + (base + t) * GR_G;
            float* oh = p.dgh + (base + t) * GR_G;
            oi[j] = a_r; oi[RN_H + j] = a_z; oi[2 * RN_H + j] = a_n;
            oh[j] = a_r; oh[RN_H + j] = a_z; oh[2 * RN_H + j] = a_nh;
        }
        __syncthreads();
        if (s > 0) part[qd][k] = dot_gate_grads(wt, dGs + qd * RN_H);        // (the same for the whole block)
        __syncthreads();
        if (s > 0 && tid < RN_H) dh_rec = dh_z + sum_partials<GR_G>(part, tid);
    }
    for (int t = len; t < p.Tmax; ++t) {
        p.dgi[(base + t) * GR_G + tid] = 0.f;
        p.dgh[(base + t) * GR_G + tid] = 0.f;
    }
}

// dbias[d][row] = sum over the n = B * Tmax positions of dg[d][.][row], in index order (one thread per (d, row): coalesced rows);
// blockIdx.y picks (dgi -> d b_ih) or (dgh -> d b_hh): the GRU's two differ (the n block of dgh carries the factor r), the LSTM has
// one dgates / dbias and leaves the other slot NULL.
template <int G>
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ dgi, const float* __restrict__ dgh, int n,
                                                        float* __restrict__ db_ih, float* __restrict__ db_hh) {
    const float* dg = blockIdx.y ? dgh : dgi;
    float* dbias = blockIdx.y ? db_hh : db_ih;
    if (!dbias) return;                                          // (the same for the whole block)
    const int idx = blockIdx.x * 256 + threadIdx.x;              // < 2 * G
    const int d = idx / G, row = idx - d * G;
    const float* src = dg + (size_t)d * n * G + row;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        a0 += src[(size_t)i * G]; a1 += src[(size_t)(i + 1) * G]; a2 += src[(size_t)(i + 2) * G]; a3 += src[(size_t)(i + 3) * G];
    }
    for (; i < n; ++i) a0 += src[(size_t)i * G];
    dbias[idx] = (a0 + a1) + (a2 + a3);
}

// embedding_bwd_kernel: one block per position (b, t).  A block whose token already occurs at an earlier valid position leaves; the
// others own their token's row: they add the (masked, scaled) dx rows of every position that holds the token, in index order, and
// add the sum to demb[tok].  B * Tmax <= 2048 positions: the all-pairs token compare is one pass per block.
struct EmbBwdP {
    const long long* cap; const float* dx; const uint8_t* mask; float scale; float* demb;
    int B, T, Tmax, V, E;
    int lens[RN_BMAX];
};

__global__ __launch_bounds__(256) void embedding_bwd_kernel(const EmbBwdP p) {
    __shared__ unsigned char match[RN_BMAX * RN_TMAX];
    __shared__ int lens[RN_BMAX];
    const int tid = threadIdx.x, pos = blockIdx.x, b = pos / p.Tmax, t = pos - b * p.Tmax;
    if (t >= min(max(p.lens[b], 0), p.Tmax)) return;           // (the same for the whole block)
    if (tid < RN_BMAX) lens[tid] = tid < p.B ? min(max(p.lens[tid], 0), p.Tmax) : 0;
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

// ------------------------------------------------------------------------------------------------ host checks
// the captions' lengths, checked against [0, Tmax], into a kernel's argument block
int copy_lens(int (&lens)[RN_BMAX], const int* lens_host, int B, int Tmax) {
    if (!lens_host) return MOGAN_ERR_SHAPE;
    for (int i = 0; i < B; ++i) { if (lens_host[i] < 0 || lens_host[i] > Tmax) return MOGAN_ERR_SHAPE; lens[i] = lens_host[i]; }
    return 0;
}

// the checks of the four forward entries; fills p (everything but the cell's own and the training fields)
int fill_forward(RnnP& p, const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                 const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0, float* words,
                 float* sent, int B, int T, int Tmax, int V, int E, int H) {
    if (!captions || !lens_host || !emb || !w_ih || !w_hh || !b_ih || !b_hh || !words || !sent) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > RN_BMAX || H != RN_H || T <= 0 || Tmax <= 0 || Tmax > T || Tmax > RN_TMAX || E <= 0 || E > RN_EMAX || (E % 4) || V <= 0)
        return MOGAN_ERR_SHAPE;
    p.cap = captions; p.emb = emb; p.h0 = h0; p.words = words; p.sent = sent;
    p.B = B; p.T = T; p.Tmax = Tmax; p.V = V; p.E = E;
    p.scale = 1.f;
    for (int d = 0; d < 2; ++d) {
        if (!w_ih[d] || !w_hh[d] || !b_ih[d] || !b_hh[d] || (((uintptr_t)w_ih[d] | (uintptr_t)w_hh[d]) & 15)) return MOGAN_ERR_SHAPE;
        p.w_ih[d] = w_ih[d]; p.w_hh[d] = w_hh[d]; p.b_ih[d] = b_ih[d]; p.b_hh[d] = b_hh[d];
    }
    return copy_lens(p.lens, lens_host, B, Tmax);
}

// the checks of the two backward entries; fills p (everything but the cell's own fields)
int fill_backward(RnnBwdP& p, const float* dwords, const float* dsent, const int* lens_host, const float* gates, const float* hprev,
                  const float* const* w_hh, int B, int Tmax, int H) {
    if (!lens_host || !gates || !hprev || !w_hh || !w_hh[0] || !w_hh[1]) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > RN_BMAX || H != RN_H || Tmax <= 0 || Tmax > RN_TMAX) return MOGAN_ERR_SHAPE;
    p.dwords = dwords; p.dsent = dsent; p.gates = gates; p.hprev = hprev;
    p.w_hh[0] = w_hh[0]; p.w_hh[1] = w_hh[1]; p.B = B; p.Tmax = Tmax;
    return copy_lens(p.lens, lens_host, B, Tmax);
}

}  // namespace

extern "C" {

int mogan_lstm_encoder_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                           const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                           const float* c0, float* words, float* sent, int B, int T, int Tmax, int V, int E, int H,
                           hipStream_t stream) {
    LstmP p{};
    if (int rc = fill_forward(p, captions, lens_host, emb, w_ih, w_hh, b_ih, b_hh, h0, words, sent, B, T, Tmax, V, E, H)) return rc;
    p.c0 = c0;
    hipLaunchKernelGGL(lstm_encoder_kernel<false>, dim3(2 * B), dim3(LS_G), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_lstm_encoder_train_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                                 const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                                 const float* c0, const uint8_t* keep_mask, float scale, float* words, float* sent, float* x,
                                 float* gates, float* cells, float* hprev, int B, int T, int Tmax, int V, int E, int H,
                                 hipStream_t stream) {
    if (!x || !gates || !cells || !hprev) return MOGAN_ERR_SHAPE;
    LstmP p{};
    if (int rc = fill_forward(p, captions, lens_host, emb, w_ih, w_hh, b_ih, b_hh, h0, words, sent, B, T, Tmax, V, E, H)) return rc;
    p.c0 = c0; p.mask = keep_mask; p.scale = scale; p.x = x; p.gates = gates; p.cells = cells; p.hprev = hprev;
    hipLaunchKernelGGL(lstm_encoder_kernel<true>, dim3(2 * B), dim3(LS_G), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_lstm_encoder_bwd(const float* dwords, const float* dsent, const int* lens_host, const float* gates, const float* cells,
                           const float* hprev, const float* c0, const float* const* w_hh, float* dgates, float* dbias, int B,
                           int Tmax, int H, hipStream_t stream) {
    if (!cells || !dgates) return MOGAN_ERR_SHAPE;
    LstmBwdP p{};
    if (int rc = fill_backward(p, dwords, dsent, lens_host, gates, hprev, w_hh, B, Tmax, H)) return rc;
    p.cells = cells; p.c0 = c0; p.dg = dgates;
    hipLaunchKernelGGL(lstm_encoder_bwd_kernel, dim3(2 * B), dim3(LS_G), 0, stream, p);
    if (dbias)
        hipLaunchKernelGGL(bias_grad_kernel<LS_G>, dim3(2 * LS_G / 256, 2), dim3(256), 0, stream, (const float*)dgates,
                           (const float*)nullptr, B * Tmax, dbias, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_gru_encoder_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                          const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                          float* words, float* sent, int B, int T, int Tmax, int V, int E, int H, hipStream_t stream) {
    GruP p{};
    if (int rc = fill_forward(p, captions, lens_host, emb, w_ih, w_hh, b_ih, b_hh, h0, words, sent, B, T, Tmax, V, E, H)) return rc;
    hipLaunchKernelGGL(gru_encoder_kernel<false>, dim3(2 * B), dim3(GR_G), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_gru_encoder_train_fwd(const long long* captions, const int* lens_host, const float* emb, const float* const* w_ih,
                                const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                                const uint8_t* keep_mask, float scale, float* words, float* sent, float* x, float* gates, float* hn,
                                float* hprev, int B, int T, int Tmax, int V, int E, int H, hipStream_t stream) {
    if (!x || !gates || !hn || !hprev) return MOGAN_ERR_SHAPE;
    GruP p{};
    if (int rc = fill_forward(p, captions, lens_host, emb, w_ih, w_hh, b_ih, b_hh, h0, words, sent, B, T, Tmax, V, E, H)) return rc;
    p.mask = keep_mask; p.scale = scale; p.x = x; p.gates = gates; p.hn = hn; p.hprev = hprev;
    hipLaunchKernelGGL(gru_encoder_kernel<true>, dim3(2 * B), dim3(GR_G), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_gru_encoder_bwd(const float* dwords, const float* dsent, const int* lens_host, const float* gates, const float* hn,
                          const float* hprev, const float* const* w_hh, float* dgi, float* dgh, float* dbias_ih, float* dbias_hh,
                          int B, int Tmax, int H, hipStream_t stream) {
    if (!hn || !dgi || !dgh) return MOGAN_ERR_SHAPE;
    GruBwdP p{};
    if (int rc = fill_backward(p, dwords, dsent, lens_host, gates, hprev, w_hh, B, Tmax, H)) return rc;
    p.hn = hn; p.dgi = dgi; p.dgh = dgh;
    hipLaunchKernelGGL(gru_encoder_bwd_kernel, dim3(2 * B), dim3(GR_G), 0, stream, p);
    if (dbias_ih || dbias_hh)
        hipLaunchKernelGGL(bias_grad_kernel<GR_G>, dim3(2 * GR_G / 256, 2), dim3(256), 0, stream, (const float*)dgi, (const float*)dgh,
                           B * Tmax, dbias_ih, dbias_hh);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

int mogan_embedding_bwd(const long long* captions, const int* lens_host, const float* dx, const uint8_t* keep_mask, float scale,
                        float* demb, int B, int T, int Tmax, int V, int E, hipStream_t stream) {
    if (!captions || !lens_host || !dx || !demb) return MOGAN_ERR_SHAPE;
    if (B <= 0 || B > RN_BMAX || T <= 0 || Tmax <= 0 || Tmax > T || Tmax > RN_TMAX || E <= 0 || E > RN_EMAX || (E % 4) || V <= 0)
        return MOGAN_ERR_SHAPE;
    EmbBwdP p{};
    p.cap = captions; p.dx = dx; p.mask = keep_mask; p.scale = scale; p.demb = demb;
    p.B = B; p.T = T; p.Tmax = Tmax; p.V = V; p.E = E;
    if (int rc = copy_lens(p.lens, lens_host, B, Tmax)) return rc;
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3(B * Tmax), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH;
}

}  // extern "C"
