// Centralized critic (reference learner/critic.py:7-87) and the DDPG update pieces around it (reference
// learner/gnn_ddpg.py:93-100,169-222): the whole critic forward / backward as one workgroup per sample, the composed
// path's GroupNorm+ReLU pair, the broadcast MSE of the critic loss, the policy loss and the soft target update.
//
// Built with -ffp-contract=off (build.py PER_FILE_FLAGS) so mgp_soft_update rounds like torch's two multiplies and one add;
// the critic loops spell their fused multiply-adds out (__fmaf_rn).
#include <math.h>
#include "mgp_common.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = CR_THREADS / MGP_WAVE;
constexpr int CR_CB = 8;                               // channels per thread item of the aggregation loops
constexpr size_t CR_LDS_MAX = 160 * 1024;

struct CriticArgs {
    const float* W[MGP_MAX_LAYERS];                    // (out, K, C_in): rows in (tap, channel) order
    const float* bias[MGP_MAX_LAYERS];
    const float* gamma[MGP_MAX_LAYERS];                // GroupNorm affine of the hidden layers
    const float* beta[MGP_MAX_LAYERS];
    int dims[MGP_MAX_LAYERS + 1];
    int L, ns, K, N;
    int cp, hp;                                        // LDS row counts: widest layer input (padded to CR_CB), widest output
};

struct CriticGrads {
    float* dW[MGP_MAX_LAYERS];
    float* db[MGP_MAX_LAYERS];
    float* dgamma[MGP_MAX_LAYERS];
    float* dbeta[MGP_MAX_LAYERS];
    long woff[MGP_MAX_LAYERS], boff[MGP_MAX_LAYERS], goff[MGP_MAX_LAYERS], beoff[MGP_MAX_LAYERS];
    long P;                                            // parameter floats per sample in the workspace
};

// ------------------------------------------------------------------------------------------------ host-side plan
bool critic_dims_ok(const int* dims, int L, int K, int N)
{
    if (dims == nullptr || L < 1 || L > MGP_MAX_LAYERS || K <= 0 || N <= 0) return false;
    for (int i = 0; i <= L; ++i) if (dims[i] <= 0) return false;
    return dims[L] == 1;
}

void critic_rows(const int* dims, int L, int& cp, int& hp)
{
    int c = 0, h = 0;
    for (int l = 0; l < L; ++l) { c = c > dims[l] ? c : dims[l]; h = h > dims[l + 1] ? h : dims[l + 1]; }
    cp = (c + CR_CB - 1) / CR_CB * CR_CB;
    hp = h;
}

size_t critic_fwd_lds(const int* dims, int L, int N)
{
    int cp, hp;
    critic_rows(dims, L, cp, hp);
    return (size_t)(2 * cp + hp) * N * sizeof(float);
}

size_t critic_bwd_lds(const int* dims, int L, int N)
{
    int cp, hp;
    critic_rows(dims, L, cp, hp);
    return (size_t)(3 * cp + hp) * N * sizeof(float);
}

// saved floats of ONE sample: the input planes, then per hidden layer pre-norm y (C,N), mean (C), rstd (C), post-ReLU a (C,N)
long critic_saved_per_sample(const int* dims, int L, int N)
{
    long s = (long)dims[0] * N;
    for (int l = 0; l + 1 < L; ++l) s += 2L * dims[l + 1] * N + 2L * dims[l + 1];
    return s;
}

long critic_params(const int* dims, int L, int K)
{
    long p = 0;
    for (int l = 0; l < L; ++l) p += (long)dims[l + 1] * K * dims[l] + dims[l + 1];
    for (int l = 0; l + 1 < L; ++l) p += 2L * dims[l + 1];
    return p;
}

// ------------------------------------------------------------------------------------------------ device helpers
// Z[c,n] = sum_m X[c,m] G[m,n] for c < C (X, Z in LDS, G one (N,N) slice in global memory, L2-resident across the batch)
__device__ __forceinline__ void cr_agg(const float* __restrict__ X, const float* __restrict__ G, float* __restrict__ Z,
                                       int C, int N)
{
    const int CG = (C + CR_CB - 1) / CR_CB;
    for (int idx = threadIdx.x; idx < N * CG; idx += CR_THREADS) {
        const int n = idx % N, cg = idx / N;
        const int c0 = cg * CR_CB;
        float z[CR_CB];
#pragma unroll
        for (int j = 0; j < CR_CB; ++j) z[j] = 0.0f;
        for (int m = 0; m < N; ++m) {
            const float g = G[(long)m * N + n];
#pragma unroll
            for (int j = 0; j < CR_CB; ++j) z[j] = __fmaf_rn(X[(c0 + j) * N + m], g, z[j]);   // rows >= C: padding, discarded
        }
#pragma unroll
        for (int j = 0; j < CR_CB; ++j)
            if (c0 + j < C) Z[(c0 + j) * N + n] = z[j];
    }
}

// D[c,m] (+)= sum_n dZ[c,n] G[m,n]   (the transpose product: the backward of cr_agg)
__device__ __forceinline__ void cr_agg_t(const float* __restrict__ dZ, const float* __restrict__ G, float* __restrict__ D,
                                         int C, int N, bool accumulate)
{
    const int CG = (C + CR_CB - 1) / CR_CB;
    for (int idx = threadIdx.x; idx < N * CG; idx += CR_THREADS) {
        const int m = idx % N, cg = idx / N;
        const int c0 = cg * CR_CB;
        float z[CR_CB];
#pragma unroll
        for (int j = 0; j < CR_CB; ++j) z[j] = 0.0f;
        const float* Gm = G + (long)m * N;
        for (int n = 0; n < N; ++n) {
            const float g = Gm[n];
#pragma unroll
            for (int j = 0; j < CR_CB; ++j) z[j] = __fmaf_rn(dZ[(c0 + j) * N + n], g, z[j]);
        }
#pragma unroll
        for (int j = 0; j < CR_CB; ++j)
            if (c0 + j < C) D[(c0 + j) * N + m] = accumulate ? D[(c0 + j) * N + m] + z[j] : z[j];
    }
}

// GroupNorm(C, C) + ReLU of one (sample, channel) row held by one wave: statistics in fp64, two passes (biased variance)
__device__ __forceinline__ void cr_gn_relu_row(const float* __restrict__ y, float* __restrict__ a, int N, float gamma,
                                               float beta, float eps, float& mean_out, float& rstd_out)
{
    const int lane = threadIdx.x & (MGP_WAVE - 1);
    double s = 0.0;
    for (int n = lane; n < N; n += MGP_WAVE) s += (double)y[n];
    const double mean = mgp_wave_sum(s) / (double)N;
    double q = 0.0;
    for (int n = lane; n < N; n += MGP_WAVE) { const double d = (double)y[n] - mean; q += d * d; }
    const double var = mgp_wave_sum(q) / (double)N;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float meanf = (float)mean;
    for (int n = lane; n < N; n += MGP_WAVE) {
        const float v = __fmaf_rn((y[n] - meanf) * rstd, gamma, beta);
        a[n] = v > 0.0f ? v : 0.0f;
    }
    mean_out = meanf;
    rstd_out = rstd;
}

// backward of one GroupNorm+ReLU row: da (the gradient of the post-ReLU plane) -> dy; returns sum(g) and sum(g xhat)
// (g = da masked by the ReLU) for dbeta / dgamma
__device__ __forceinline__ void cr_gn_relu_row_bwd(const float* __restrict__ da, const float* __restrict__ y,
                                                   const float* __restrict__ a, float mean, float rstd, float gamma,
                                                   float* __restrict__ dy, int N, float& sg, float& sgx)
{
    const int lane = threadIdx.x & (MGP_WAVE - 1);
    double s1 = 0.0, s2 = 0.0;
    for (int n = lane; n < N; n += MGP_WAVE) {
        const float g = a[n] > 0.0f ? da[n] : 0.0f;
        const float xh = (y[n] - mean) * rstd;
        s1 += (double)g;
        s2 += (double)g * (double)xh;
    }
    s1 = mgp_wave_sum(s1);
    s2 = mgp_wave_sum(s2);
    const float m1 = (float)(s1 * (double)gamma / (double)N);      // mean of dxhat
    const float m2 = (float)(s2 * (double)gamma / (double)N);      // mean of dxhat * xhat
    for (int n = lane; n < N; n += MGP_WAVE) {
        const float g = a[n] > 0.0f ? da[n] : 0.0f;
        const float xh = (y[n] - mean) * rstd;
        dy[n] = rstd * (g * gamma - m1 - xh * m2);
    }
    sg = (float)s1;
    sgx = (float)s2;
}

// ------------------------------------------------------------------------------------------------ fused forward
__global__ __launch_bounds__(CR_THREADS)
void critic_fwd_kernel(const float* __restrict__ S, const float* __restrict__ A, const float* __restrict__ G,
                       const CriticArgs p, float* __restrict__ Q, float* __restrict__ saved, long saved_per)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = p.N, K = p.K, b = blockIdx.x;
    float* cur = smem;                        // layer input (C, N)
    float* Z = cur + p.cp * N;                // one tap's aggregation (C, N)
    float* acc = Z + p.cp * N;                // layer output (O, N)
    const int C0 = p.dims[0], na = C0 - p.ns;
    float* sv = saved != nullptr ? saved + (long)b * saved_per : nullptr;
    for (int i = threadIdx.x; i < C0 * N; i += CR_THREADS) {
        const int c = i / N, n = i % N;
        const float v = c < p.ns ? S[((long)b * p.ns + c) * N + n] : A[((long)b * na + (c - p.ns)) * N + n];
        cur[i] = v;
        if (sv != nullptr) sv[i] = v;
    }
    if (sv != nullptr) sv += (long)C0 * N;
    const float* Gb = G + (long)b * K * N * N;
    __syncthreads();
    for (int l = 0; l < p.L; ++l) {
        const int C = p.dims[l], O = p.dims[l + 1];
        const float* W = p.W[l];
        for (int k = 0; k < K; ++k) {
            cr_agg(cur, Gb + (long)k * N * N, Z, C, N);
            __syncthreads();
            for (int i = threadIdx.x; i < O * N; i += CR_THREADS) {
                const int o = i / N, n = i % N;
                const float* w = W + ((long)o * K + k) * C;
                float s = k == 0 ? p.bias[l][o] : acc[i];
                for (int c = 0; c < C; ++c) s = __fmaf_rn(w[c], Z[c * N + n], s);
                acc[i] = s;
            }
            __syncthreads();
        }
        if (l + 1 == p.L) {
            for (int n = threadIdx.x; n < N; n += CR_THREADS) Q[(long)b * N + n] = acc[n];
            break;
        }
        // GroupNorm + ReLU, one wave per channel; the post-ReLU planes become the next layer's input
        const int wave = threadIdx.x / MGP_WAVE, lane = threadIdx.x & (MGP_WAVE - 1);
        for (int o = wave; o < O; o += CR_WAVES) {
            float mean, rstd;
            cr_gn_relu_row(acc + o * N, cur + o * N, N, p.gamma[l][o], p.beta[l][o], 1e-5f, mean, rstd);
            if (sv != nullptr) {
                for (int n = lane; n < N; n += MGP_WAVE) {
                    sv[(long)o * N + n] = acc[o * N + n];
                    sv[(long)O * N + 2 * O + (long)o * N + n] = cur[o * N + n];
                }
                if (lane == 0) { sv[(long)O * N + o] = mean; sv[(long)O * N + O + o] = rstd; }
            }
        }
        if (sv != nullptr) sv += 2L * O * N + 2L * O;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ fused backward
// One workgroup per sample, layers in reverse.  Parameter gradients of the sample go to ws[b * P ...] in the module's
// parameter order; critic_reduce_kernel sums them over the batch in sample order (no atomics: identical calls, identical bits).
__global__ __launch_bounds__(CR_THREADS)
void critic_bwd_kernel(const float* __restrict__ dQ, const float* __restrict__ G, const float* __restrict__ saved,
                       long saved_per, const CriticArgs p, const CriticGrads gr, bool want_params,
                       float* __restrict__ dAct, float* __restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = p.N, K = p.K, L = p.L, b = blockIdx.x;
    float* xin = smem;                        // layer input (C, N)
    float* Z = xin + p.cp * N;                // tap aggregation, then its gradient (C, N)
    float* dx = Z + p.cp * N;                 // gradient of the layer input (C, N)
    float* g = dx + p.cp * N;                 // gradient of the layer's pre-norm output (O, N)
    const int wave = threadIdx.x / MGP_WAVE, lane = threadIdx.x & (MGP_WAVE - 1);
    const float* sv0 = saved + (long)b * saved_per;
    float* wsb = ws != nullptr ? ws + (long)b * gr.P : nullptr;
    const float* Gb = G + (long)b * K * N * N;
    // per hidden layer h: offset of its (y, mean, rstd, a) block in the sample's saved record
    long hoff[MGP_MAX_LAYERS];
    {
        long o = (long)p.dims[0] * N;
        for (int h = 0; h + 1 < L; ++h) { hoff[h] = o; o += 2L * p.dims[h + 1] * N + 2L * p.dims[h + 1]; }
    }
    for (int n = threadIdx.x; n < N; n += CR_THREADS) g[n] = dQ[(long)b * N + n];
    for (int l = L - 1; l >= 0; --l) {
        const int C = p.dims[l], O = p.dims[l + 1];
        const float* src = l == 0 ? sv0 : sv0 + hoff[l - 1] + (long)C * N + 2L * C;     // post-ReLU planes of layer l-1
        for (int i = threadIdx.x; i < C * N; i += CR_THREADS) xin[i] = src[i];
        __syncthreads();
        const bool need_dx = l > 0 || dAct != nullptr;
        if (want_params) {
            for (int o = wave; o < O; o += CR_WAVES) {
                float s = 0.0f;
                for (int n = lane; n < N; n += MGP_WAVE) s += g[o * N + n];
                s = mgp_wave_sum(s);
                if (lane == 0) wsb[gr.boff[l] + o] = s;
            }
        }
        const float* W = p.W[l];
        for (int k = 0; k < K; ++k) {
            const float* Gk = Gb + (long)k * N * N;
            if (want_params) {
                cr_agg(xin, Gk, Z, C, N);
                __syncthreads();
                for (int i = threadIdx.x; i < O * C; i += CR_THREADS) {
                    const int o = i / C, c = i % C;
                    float s = 0.0f;
                    for (int n = 0; n < N; ++n) s = __fmaf_rn(g[o * N + n], Z[c * N + n], s);
                    wsb[gr.woff[l] + ((long)o * K + k) * C + c] = s;
                }
                __syncthreads();
            }
            if (need_dx) {
                for (int i = threadIdx.x; i < C * N; i += CR_THREADS) {
                    const int c = i / N, n = i % N;
                    float s = 0.0f;
                    for (int o = 0; o < O; ++o) s = __fmaf_rn(W[((long)o * K + k) * C + c], g[o * N + n], s);
                    Z[i] = s;
                }
                __syncthreads();
                cr_agg_t(Z, Gk, dx, C, N, k > 0);
                __syncthreads();
            }
        }
        if (l == 0) {
            if (dAct != nullptr) {
                const int na = C - p.ns;
                for (int i = threadIdx.x; i < na * N; i += CR_THREADS)
                    dAct[(long)b * na * N + i] = dx[p.ns * N + i];
            }
            break;
        }
        // GroupNorm+ReLU of hidden layer l-1: dx is the gradient of its post-ReLU planes; g becomes its pre-norm gradient
        const float* y = sv0 + hoff[l - 1];
        const float* mean = y + (long)C * N;
        const float* rstd = mean + C;
        const float* a = rstd + C;
        for (int c = wave; c < C; c += CR_WAVES) {
            float sg, sgx;
            cr_gn_relu_row_bwd(dx + c * N, y + (long)c * N, a + (long)c * N, mean[c], rstd[c], p.gamma[l - 1][c],
                               g + c * N, N, sg, sgx);
            if (want_params && lane == 0) { wsb[gr.goff[l - 1] + c] = sgx; wsb[gr.beoff[l - 1] + c] = sg; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256)
void critic_reduce_kernel(const float* __restrict__ ws, const CriticGrads gr, int L, int B)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= gr.P) return;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) s += ws[(long)b * gr.P + i];
    for (int l = 0; l < L; ++l) {
        if (i >= gr.woff[l] && i < gr.boff[l]) { gr.dW[l][i - gr.woff[l]] = s; return; }
        const long bend = l + 1 < L ? gr.woff[l + 1] : gr.goff[0];
        if (i >= gr.boff[l] && i < bend) { gr.db[l][i - gr.boff[l]] = s; return; }
    }
    for (int l = 0; l + 1 < L; ++l) {
        if (i >= gr.goff[l] && i < gr.beoff[l]) { gr.dgamma[l][i - gr.goff[l]] = s; return; }
        const long e = l + 2 < L ? gr.goff[l + 1] : gr.P;
        if (i >= gr.beoff[l] && i < e) { gr.dbeta[l][i - gr.beoff[l]] = s; return; }
    }
}

// ------------------------------------------------------------------------------------------------ composed path
__global__ __launch_bounds__(256)
void gn_relu_fwd_kernel(const float* __restrict__ Y, const float* __restrict__ gamma, const float* __restrict__ beta,
                        float* __restrict__ A, float* __restrict__ mean, float* __restrict__ rstd, int B, int C, int N,
                        float eps)
{
    const long row = (long)blockIdx.x * 4 + threadIdx.x / MGP_WAVE;
    if (row >= (long)B * C) return;
    const int c = (int)(row % C);
    float mu, rs;
    cr_gn_relu_row(Y + row * N, A + row * N, N, gamma[c], beta[c], eps, mu, rs);
    if ((threadIdx.x & (MGP_WAVE - 1)) == 0) {
        if (mean != nullptr) mean[row] = mu;
        if (rstd != nullptr) rstd[row] = rs;
    }
}

// dA is (B, taps, C, N): the gradient of the post-ReLU planes is its sum over the taps (the next layer's aggregation read
// every plane once per tap)
__global__ __launch_bounds__(256)
void gn_relu_bwd_kernel(const float* __restrict__ dA, int taps, const float* __restrict__ Y, const float* __restrict__ A,
                        const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                        float* __restrict__ dY, float* __restrict__ ws, int B, int C, int N)
{
    extern __shared__ float sda[];            // 4 rows of N
    const int w = threadIdx.x / MGP_WAVE, lane = threadIdx.x & (MGP_WAVE - 1);
    const long row = (long)blockIdx.x * 4 + w;
    if (row >= (long)B * C) return;
    const long b = row / C;
    const int c = (int)(row % C);
    float* da = sda + w * N;
    for (int n = lane; n < N; n += MGP_WAVE) {
        float s = 0.0f;
        for (int t = 0; t < taps; ++t) s += dA[((b * taps + t) * C + c) * N + n];
        da[n] = s;
    }
    float sg, sgx;
    cr_gn_relu_row_bwd(da, Y + row * N, A + row * N, mean[row], rstd[row], gamma[c], dY + row * N, N, sg, sgx);
    if (ws != nullptr && lane == 0) { ws[2 * row] = sgx; ws[2 * row + 1] = sg; }
}

__global__ __launch_bounds__(256)
void gn_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dgamma, float* __restrict__ dbeta, int B, int C)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float sgx = 0.0f, sg = 0.0f;
    for (int b = 0; b < B; ++b) { sgx += ws[2 * ((long)b * C + c)]; sg += ws[2 * ((long)b * C + c) + 1]; }
    dgamma[c] = sgx;
    dbeta[c] = sg;
}

__global__ __launch_bounds__(256)
void tap_sum_kernel(const float* __restrict__ X, float* __restrict__ out, int B, int T, int C, int c0, int Cs, int N)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * Cs * N) return;
    const long b = i / ((long)Cs * N);
    const int r = (int)(i % ((long)Cs * N));
    const int c = r / N, n = r % N;
    float s = 0.0f;
    for (int t = 0; t < T; ++t) s += X[((b * T + t) * C + c0 + c) * N + n];
    out[i] = s;
}

// ------------------------------------------------------------------------------------------------ DDPG losses, soft update
constexpr int LS_THREADS = 1024;

// F.mse_loss(Q (B,1,N), r + gamma nd Q' (B,B,N)) (gnn_ddpg.py:195,200): the target broadcasts over a second batch axis j.
// With c_j = gamma nd_j (fp32, as torch forms it):  sum_j (q - r_j - c_j t)^2 = B q^2 + S_rr + t^2 S_cc - 2 q S_r - 2 q t S_c
// + 2 t S_rc; dQ[i,n] = 2 / (B B N) (B q - S_r - t S_c).  Sums over j in fp64, in sample order.
__global__ __launch_bounds__(LS_THREADS)
void critic_loss_kernel(const float* __restrict__ Q, const float* __restrict__ Qt, const float* __restrict__ r,
                        const float* __restrict__ nd, float gamma, float* __restrict__ loss, float* __restrict__ dQ,
                        int B, int N)
{
    __shared__ double sj[5];
    __shared__ double sh[LS_THREADS / MGP_WAVE];
    if (threadIdx.x == 0) {
        double s_r = 0.0, s_c = 0.0, s_rr = 0.0, s_cc = 0.0, s_rc = 0.0;
        for (int j = 0; j < B; ++j) {
            const double rj = (double)r[j], cj = (double)(gamma * nd[j]);
            s_r += rj; s_c += cj; s_rr += rj * rj; s_cc += cj * cj; s_rc += rj * cj;
        }
        sj[0] = s_r; sj[1] = s_c; sj[2] = s_rr; sj[3] = s_cc; sj[4] = s_rc;
    }
    __syncthreads();
    const double s_r = sj[0], s_c = sj[1], s_rr = sj[2], s_cc = sj[3], s_rc = sj[4];
    const double Bd = (double)B, inv = 1.0 / (Bd * Bd * (double)N);
    double acc = 0.0;
    for (long i = threadIdx.x; i < (long)B * N; i += LS_THREADS) {
        const double q = (double)Q[i], t = (double)Qt[i];
        acc += Bd * q * q + s_rr + t * t * s_cc - 2.0 * q * s_r - 2.0 * q * t * s_c + 2.0 * t * s_rc;
        if (dQ != nullptr) dQ[i] = (float)(2.0 * inv * (Bd * q - s_r - t * s_c));
    }
    acc = mgp_wave_sum(acc);
    if ((threadIdx.x & (MGP_WAVE - 1)) == 0) sh[threadIdx.x / MGP_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && loss != nullptr) {
        double t = 0.0;
        for (int w = 0; w < LS_THREADS / MGP_WAVE; ++w) t += sh[w];
        loss[0] = (float)(t * inv);
    }
}

// policy_loss = -mean Q(s, mu(s)) (gnn_ddpg.py:207): loss and its gradient -1 / (B N)
__global__ __launch_bounds__(LS_THREADS)
void policy_loss_kernel(const float* __restrict__ Q, float* __restrict__ loss, float* __restrict__ dQ, long n)
{
    __shared__ double sh[LS_THREADS / MGP_WAVE];
    const float g = -1.0f / (float)n;
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += LS_THREADS) {
        acc += (double)Q[i];
        if (dQ != nullptr) dQ[i] = g;
    }
    acc = mgp_wave_sum(acc);
    if ((threadIdx.x & (MGP_WAVE - 1)) == 0) sh[threadIdx.x / MGP_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && loss != nullptr) {
        double t = 0.0;
        for (int w = 0; w < LS_THREADS / MGP_WAVE; ++w) t += sh[w];
        loss[0] = (float)(-t / (double)n);
    }
}

// t.copy_(t * (1 - tau) + tau * p) (gnn_ddpg.py:93-100): two fp32 multiplies, one add, no contraction (file flag)
__global__ __launch_bounds__(256)
void soft_update_kernel(float* __restrict__ t, const float* __restrict__ p, long n, float one_m_tau, float tau)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = t[i] * one_m_tau;
    const float c = tau * p[i];
    t[i] = a + c;
}

// bias / beta are read by the forward only (the backward passes nullptr for both)
int critic_fill_args(CriticArgs& a, const float* const* W, const float* const* bias, const float* const* gamma,
                     const float* const* beta, const int* dims, int L, int n_s, int K, int N)
{
    const bool fwd = bias != nullptr;
    if (!critic_dims_ok(dims, L, K, N) || n_s <= 0 || n_s >= dims[0]) return MGP_EINVAL;
    if (W == nullptr) return MGP_EINVAL;
    for (int l = 0; l < L; ++l) {
        a.dims[l] = dims[l];
        a.W[l] = W[l];
        a.bias[l] = fwd ? bias[l] : nullptr;
        MGP_CHECK_PTR(a.W[l]);
        if (fwd) MGP_CHECK_PTR(a.bias[l]);
        a.gamma[l] = a.beta[l] = nullptr;
        if (l + 1 < L) {
            if (gamma == nullptr || (fwd && beta == nullptr)) return MGP_EINVAL;
            a.gamma[l] = gamma[l];
            MGP_CHECK_PTR(a.gamma[l]);
            if (fwd) { a.beta[l] = beta[l]; MGP_CHECK_PTR(a.beta[l]); }
        }
    }
    a.dims[L] = dims[L];
    a.L = L; a.ns = n_s; a.K = K; a.N = N;
    critic_rows(dims, L, a.cp, a.hp);
    return MGP_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int mgp_critic_supported(const int* dims, int n_layers, int B, int K, int N)
{
    if (!critic_dims_ok(dims, n_layers, K, N) || B <= 0) return 0;
    if (N > 1024) return 0;
    return critic_fwd_lds(dims, n_layers, N) <= CR_LDS_MAX && critic_bwd_lds(dims, n_layers, N) <= CR_LDS_MAX ? 1 : 0;
}

extern "C" long mgp_critic_saved_floats(const int* dims, int n_layers, int B, int K, int N)
{
    if (!critic_dims_ok(dims, n_layers, K, N) || B <= 0) return -1;
    return (long)B * critic_saved_per_sample(dims, n_layers, N);
}

extern "C" long mgp_critic_bwd_workspace(const int* dims, int n_layers, int B, int K, int N)
{
    if (!critic_dims_ok(dims, n_layers, K, N) || B <= 0) return -1;
    return (long)B * critic_params(dims, n_layers, K);
}

extern "C" int mgp_critic_fwd(const float* S, const float* A, const float* G, const float* const* W,
                              const float* const* bias, const float* const* gamma, const float* const* beta,
                              const int* dims, int n_layers, int n_s, float* Q, float* saved, int B, int K, int N,
                              void* stream)
{
    if (B <= 0) return B == 0 ? MGP_OK : MGP_EINVAL;
    CriticArgs a;
    const int rc = critic_fill_args(a, W, bias, gamma, beta, dims, n_layers, n_s, K, N);
    if (rc != MGP_OK) return rc;
    MGP_CHECK_PTR(S); MGP_CHECK_PTR(A); MGP_CHECK_PTR(G); MGP_CHECK_PTR(Q);
    if (saved != nullptr && (reinterpret_cast<uintptr_t>(saved) & 3u)) return MGP_EALIGN;
    if (!mgp_critic_supported(dims, n_layers, B, K, N)) return MGP_EUNSUPPORTED;
    mgp_clear_error();
    const size_t lds = critic_fwd_lds(dims, n_layers, N);
    if (mgp_allow_dyn_lds((const void*)critic_fwd_kernel, lds) != hipSuccess) return mgp_launch_status();
    hipLaunchKernelGGL(critic_fwd_kernel, dim3(B), dim3(CR_THREADS), lds, static_cast<hipStream_t>(stream),
                       S, A, G, a, Q, saved, critic_saved_per_sample(dims, n_layers, N));
    return mgp_launch_status();
}

extern "C" int mgp_critic_bwd(const float* dQ, const float* G, const float* saved, const float* const* W,
                              const float* const* gamma, const int* dims, int n_layers, int n_s,
                              float* const* dW, float* const* db, float* const* dgamma, float* const* dbeta,
                              float* dActions, float* workspace, int B, int K, int N, void* stream)
{
    if (B <= 0) return B == 0 ? MGP_OK : MGP_EINVAL;
    CriticArgs a;
    int rc = critic_fill_args(a, W, nullptr, gamma, nullptr, dims, n_layers, n_s, K, N);
    if (rc != MGP_OK) return rc;
    MGP_CHECK_PTR(dQ); MGP_CHECK_PTR(G); MGP_CHECK_PTR(saved);
    const bool want_params = dW != nullptr;
    if (!want_params && dActions == nullptr) return MGP_EINVAL;
    if (dActions != nullptr && (reinterpret_cast<uintptr_t>(dActions) & 3u)) return MGP_EALIGN;
    if (!mgp_critic_supported(dims, n_layers, B, K, N)) return MGP_EUNSUPPORTED;
    CriticGrads gr;
    long off = 0;
    for (int l = 0; l < n_layers; ++l) {
        gr.woff[l] = off; off += (long)dims[l + 1] * K * dims[l];
        gr.boff[l] = off; off += dims[l + 1];
    }
    for (int l = 0; l + 1 < n_layers; ++l) {
        gr.goff[l] = off; off += dims[l + 1];
        gr.beoff[l] = off; off += dims[l + 1];
    }
    if (n_layers == 1) gr.goff[0] = off;
    gr.P = off;
    for (int l = 0; l < MGP_MAX_LAYERS; ++l) gr.dW[l] = gr.db[l] = gr.dgamma[l] = gr.dbeta[l] = nullptr;
    if (want_params) {
        if (db == nullptr || workspace == nullptr || (n_layers > 1 && (dgamma == nullptr || dbeta == nullptr))) return MGP_EINVAL;
        MGP_CHECK_PTR(workspace);
        for (int l = 0; l < n_layers; ++l) {
            gr.dW[l] = dW[l]; gr.db[l] = db[l];
            MGP_CHECK_PTR(gr.dW[l]); MGP_CHECK_PTR(gr.db[l]);
            if (l + 1 < n_layers) {
                gr.dgamma[l] = dgamma[l]; gr.dbeta[l] = dbeta[l];
                MGP_CHECK_PTR(gr.dgamma[l]); MGP_CHECK_PTR(gr.dbeta[l]);
            }
        }
    }
    mgp_clear_error();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = critic_bwd_lds(dims, n_layers, N);
    if (mgp_allow_dyn_lds((const void*)critic_bwd_kernel, lds) != hipSuccess) return mgp_launch_status();
    hipLaunchKernelGGL(critic_bwd_kernel, dim3(B), dim3(CR_THREADS), lds, st, dQ, G, saved,
                       critic_saved_per_sample(dims, n_layers, N), a, gr, want_params, dActions,
                       want_params ? workspace : nullptr);
    if (want_params)
        hipLaunchKernelGGL(critic_reduce_kernel, dim3((unsigned)((gr.P + 255) / 256)), dim3(256), 0, st,
                           (const float*)workspace, gr, n_layers, B);
    return mgp_launch_status();
}

extern "C" int mgp_gn_relu_fwd(const float* Y, const float* gamma, const float* beta, float* A, float* mean, float* rstd,
                               int B, int C, int N, float eps, void* stream)
{
    if (B < 0 || C <= 0 || N <= 0) return MGP_EINVAL;
    if (B == 0) return MGP_OK;
    MGP_CHECK_PTR(Y); MGP_CHECK_PTR(gamma); MGP_CHECK_PTR(beta); MGP_CHECK_PTR(A);
    mgp_clear_error();
    const long rows = (long)B * C;
    hipLaunchKernelGGL(gn_relu_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       Y, gamma, beta, A, mean, rstd, B, C, N, eps);
    return mgp_launch_status();
}

extern "C" long mgp_gn_relu_bwd_workspace(int B, int C)
{
    if (B <= 0 || C <= 0) return -1;
    return 2L * B * C;
}

extern "C" int mgp_gn_relu_bwd(const float* dA, int taps, const float* Y, const float* A, const float* mean,
                               const float* rstd, const float* gamma, float* dY, float* dgamma, float* dbeta,
                               float* workspace, int B, int C, int N, void* stream)
{
    if (B < 0 || C <= 0 || N <= 0 || taps <= 0 || N > 2048) return MGP_EINVAL;   // 4 rows of N in static-size LDS
    if (B == 0) return MGP_OK;
    MGP_CHECK_PTR(dA); MGP_CHECK_PTR(Y); MGP_CHECK_PTR(A); MGP_CHECK_PTR(mean); MGP_CHECK_PTR(rstd);
    MGP_CHECK_PTR(gamma); MGP_CHECK_PTR(dY);
    const bool params = dgamma != nullptr || dbeta != nullptr;
    if (params) { MGP_CHECK_PTR(dgamma); MGP_CHECK_PTR(dbeta); MGP_CHECK_PTR(workspace); }
    mgp_clear_error();
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long rows = (long)B * C;
    hipLaunchKernelGGL(gn_relu_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), (size_t)4 * N * sizeof(float), st,
                       dA, taps, Y, A, mean, rstd, gamma, dY, params ? workspace : nullptr, B, C, N);
    if (params)
        hipLaunchKernelGGL(gn_reduce_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st,
                           (const float*)workspace, dgamma, dbeta, B, C);
    return mgp_launch_status();
}

extern "C" int mgp_tap_sum(const float* X, float* out, int B, int T, int C, int c0, int Cs, int N, void* stream)
{
    if (B < 0 || T <= 0 || C <= 0 || N <= 0 || c0 < 0 || Cs <= 0 || c0 + Cs > C) return MGP_EINVAL;
    if (B == 0) return MGP_OK;
    MGP_CHECK_PTR(X); MGP_CHECK_PTR(out);
    mgp_clear_error();
    const long n = (long)B * Cs * N;
    hipLaunchKernelGGL(tap_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       X, out, B, T, C, c0, Cs, N);
    return mgp_launch_status();
}

extern "C" int mgp_ddpg_critic_loss(const float* Q, const float* Qt, const float* r, const float* notdone, float gamma,
                                    float* loss, float* dQ, int B, int N, void* stream)
{
    if (B <= 0 || N <= 0) return MGP_EINVAL;
    MGP_CHECK_PTR(Q); MGP_CHECK_PTR(Qt); MGP_CHECK_PTR(r); MGP_CHECK_PTR(notdone);
    if (loss == nullptr && dQ == nullptr) return MGP_EINVAL;
    mgp_clear_error();
    hipLaunchKernelGGL(critic_loss_kernel, dim3(1), dim3(LS_THREADS), 0, static_cast<hipStream_t>(stream),
                       Q, Qt, r, notdone, gamma, loss, dQ, B, N);
    return mgp_launch_status();
}

extern "C" int mgp_ddpg_policy_loss(const float* Q, float* loss, float* dQ, int B, int N, void* stream)
{
    if (B <= 0 || N <= 0) return MGP_EINVAL;
    MGP_CHECK_PTR(Q);
    if (loss == nullptr && dQ == nullptr) return MGP_EINVAL;
    mgp_clear_error();
    hipLaunchKernelGGL(policy_loss_kernel, dim3(1), dim3(LS_THREADS), 0, static_cast<hipStream_t>(stream),
                       Q, loss, dQ, (long)B * N);
    return mgp_launch_status();
}

extern "C" int mgp_soft_update(float* target, const float* source, long n, double tau, void* stream)
{
    if (n <= 0) return MGP_EINVAL;
    MGP_CHECK_PTR(target); MGP_CHECK_PTR(source);
    mgp_clear_error();
    // 1 - tau in double, then fp32: torch multiplies an fp32 tensor by the Python floats (1.0 - tau) and tau rounded to fp32
    hipLaunchKernelGGL(soft_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       target, source, n, (float)(1.0 - tau), (float)tau);
    return mgp_launch_status();
}
