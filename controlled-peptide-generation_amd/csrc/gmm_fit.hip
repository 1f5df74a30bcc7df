// Fitting the CLaSS proposal density Q(z) on the device (density_modeling.py mogQ: sklearn GaussianMixture(covariance_type='diag')
// .fit(z)), as scikit-learn 1.7 computes it:
//   k-means++ seeding     cluster._kmeans._kmeans_plusplus   (kpp_dist / kpp_search / kpp_pick, chained on the device)
//   Lloyd iterations      cluster._k_means_lloyd.lloyd_iter_chunked_dense + _k_means_common._relocate_empty_clusters_dense
//   EM iterations         mixture._gaussian_mixture: _estimate_log_gaussian_prob (diag), _e_step, _m_step, _initialize
// Element type T = float or double, the dtype of X (scikit-learn computes in the dtype of its input).  Every cross-workgroup sum is
// a per-workgroup f64 partial reduced in a fixed order: results do not depend on scheduling.
//
// Tile passes (Lloyd, EM, score): 1024 threads, 64 rows of X per tile staged in LDS, one pass over X per iteration.
//   row phase:    wave w of the 16 takes components k = w, w+16, ... for the 64 rows (one row per lane): the component's parameters
//                 are wave-uniform (scalar loads), the row comes from LDS.  Result (distance or weighted log-density) -> LDS [64][K].
//                 The E-step's expansion is accumulated in f64 for either T (its terms cancel by an order of magnitude).
//   row reduce:   16 lanes per row: argmin (Lloyd, lowest index on ties) or logsumexp -> responsibilities in place.
//   column phase: thread p of the K*D (k, d) pairs (16 per thread at most) adds the tile's sum_r w[r][k] x[r][d] (and x^2 for EM)
//                 to f64 registers; written once per workgroup at the end.
#include "cpg_internal.h"

namespace {

constexpr int GB = 1024;        // threads of the tile passes
constexpr int GR = 64;          // rows per tile
constexpr int GMAX = 128;       // largest D and K
constexpr int GPJ = GMAX * GMAX / GB;   // (k, d) pairs per thread at most
constexpr int GG = 256;         // workgroups of a tile pass at most (partials rows; fixed so workspace queries need no device)
constexpr int KPP_R = 256;      // rows per k-means++ chunk (= threads of kpp_dist)
constexpr int KPP_LMAX = 16;    // local trials per center at most

enum { M_LLOYD = 0, M_LABEL = 1, M_EM = 2, M_INIT = 3, M_SCORE = 4 };

// parameter block of a fitted mixture, element type T: w[K] logw[K] logdet[K] smp[K] means[KD] covars[KD] pchol[KD] mp[KD] prec[KD]
template <typename T> struct Params {
    T *w, *logw, *logdet, *smp, *means, *covars, *pchol, *mp, *prec;
    __host__ __device__ Params(void* base, int K, int D) {
        T* p = (T*)base;
        const size_t KD = (size_t)K * D;
        w = p; logw = p + K; logdet = p + 2 * K; smp = p + 3 * K;
        means = p + 4 * K; covars = means + KD; pchol = covars + KD; mp = pchol + KD; prec = mp + KD;
    }
};

size_t tile_lds(int D, int K, int dbytes) {
    return (size_t)GR * (D + 1) * dbytes + (size_t)GR * K * dbytes + GR * (sizeof(int) + sizeof(double)) + (size_t)K * dbytes;
}
int pass_grid(size_t n) { return (int)std::min<size_t>(GG, (n + GR - 1) / GR); }
// partial width of a pass: Lloyd sums[KD] counts[K] changed; EM srx[KD] srx2[KD] nk[K] sum log_prob_norm
__host__ __device__ inline size_t pass_width(int mode, int K, int D) { return (size_t)K * D * (mode == M_LLOYD ? 1 : 2) + K + 1; }

template <typename T>
__global__ void __launch_bounds__(GB) gmm_tile_pass(const T* __restrict__ X, size_t n, int D, int K, int mode, const T* mean,
                                                    const T* centers, const void* pblock, int32_t* labels, T* rowdist,
                                                    T* out_lpn, T* out_resp, int32_t* out_label, double* part) {
    extern __shared__ __align__(16) unsigned char smem[];
    T* xs = (T*)smem;                         // [GR][D+1]
    T* ws = xs + GR * (D + 1);                // [GR][K]
    int* lab = (int*)(ws + GR * K);           // [GR]
    double* rowv = (double*)(lab + GR);       // [GR]
    T* cn = (T*)(rowv + GR);                  // [K] squared center norms (Lloyd)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KD = K * D;
    const bool lloyd = mode == M_LLOYD || mode == M_LABEL;
    const bool cols = mode == M_LLOYD || mode == M_EM || mode == M_INIT;
    Params<T> P(const_cast<void*>(pblock), pblock ? K : 0, pblock ? D : 0);
    if (lloyd && tid < K) {
        T s = 0;
        for (int d = 0; d < D; ++d) s += centers[(size_t)tid * D + d] * centers[(size_t)tid * D + d];
        cn[tid] = s;
    }
    double acc1[GPJ], acc2[GPJ], accn = 0.0, accs = 0.0;
#pragma unroll
    for (int j = 0; j < GPJ; ++j) acc1[j] = acc2[j] = 0.0;
    const size_t ntiles = (n + GR - 1) / GR;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t row0 = t * GR;
        const int rows = (int)std::min<size_t>(GR, n - row0);
        __syncthreads();   // previous tile's LDS readers are done
        for (int i = tid; i < GR * D; i += GB) {   // rows of a tile are contiguous in X: coalesced
            const int r = i / D, d = i - r * D;
            T v = 0;
            if (r < rows) {
                v = X[row0 * D + i];
                if (mean) v = v - mean[d];   // KMeans.fit works on X - X.mean(0)
            }
            xs[r * (D + 1) + d] = v;
        }
        __syncthreads();
        // ---- row phase: one row per lane, components k = wave + 16 i
        {
            const int r = lane;
            constexpr int KPW = GMAX / 16;
            T a1[KPW], a2[KPW];
#pragma unroll
            for (int i = 0; i < KPW; ++i) a1[i] = a2[i] = 0;
            const T* xr = xs + r * (D + 1);
            if (lloyd) {
                for (int d = 0; d < D; ++d) {
                    const T x = xr[d];
#pragma unroll
                    for (int i = 0; i < KPW; ++i) {
                        const int k = wave + 16 * i;
                        if (k < K) a1[i] += x * centers[(size_t)k * D + d];
                    }
                }
#pragma unroll
                for (int i = 0; i < KPW; ++i) {
                    const int k = wave + 16 * i;
                    if (k < K) ws[r * K + k] = cn[k] + (T)-2 * a1[i];   // ||c||^2 - 2 x.c (the ||x||^2 term is common to the row)
                }
            } else if (mode == M_INIT) {
                if (wave == 0) rowv[r] = 0.0;
                const int l = (r < rows) ? labels[row0 + r] : -1;
#pragma unroll
                for (int i = 0; i < KPW; ++i) {
                    const int k = wave + 16 * i;
                    if (k < K) ws[r * K + k] = (k == l) ? (T)1 : (T)0;
                }
            } else {
                // the expansion's three terms are ~1e3 where they cancel to ~1e2: accumulated in f64 whatever T is, so the
                // responsibilities of weak components keep f64-grade accuracy on f32 storage
                double b1[KPW], b2[KPW];
#pragma unroll
                for (int i = 0; i < KPW; ++i) b1[i] = b2[i] = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double x = (double)xr[d], x2 = x * x;
#pragma unroll
                    for (int i = 0; i < KPW; ++i) {
                        const int k = wave + 16 * i;
                        if (k < K) {
                            b1[i] += x * (double)P.mp[(size_t)k * D + d];
                            b2[i] += x2 * (double)P.prec[(size_t)k * D + d];
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < KPW; ++i) {
                    const int k = wave + 16 * i;
                    if (k < K) {
                        const double lp = (double)P.smp[k] - 2.0 * b1[i] + b2[i];
                        ws[r * K + k] = (T)(-0.5 * ((double)D * 1.8378770664093453 + lp) + (double)P.logdet[k] + (double)P.logw[k]);
                    }
                }
            }
        }
        __syncthreads();
        // ---- row reduce: 16 lanes per row
        if (mode != M_INIT) {
            const int r = tid >> 4, s = tid & 15;
            T* wr = ws + r * K;
            if (lloyd) {
                T best = wr[s < K ? s : 0];
                int bi = s < K ? s : 0;
                for (int k = s + 16; k < K; k += 16)
                    if (wr[k] < best) { best = wr[k]; bi = k; }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    const T ob = __shfl_xor(best, o, 64);
                    const int oi = __shfl_xor(bi, o, 64);
                    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                }
                if (s == 0) {
                    lab[r] = r < rows ? bi : -1;
                    double ch = 0.0;
                    if (r < rows) {
                        const size_t row = row0 + r;
                        if (mode == M_LLOYD) {
                            ch = labels[row] != bi ? 1.0 : 0.0;
                            T dd = 0;   // ((X - centers_old[labels])**2).sum(1): the relocation key of empty clusters
                            for (int d = 0; d < D; ++d) {
                                const T e = xs[r * (D + 1) + d] - centers[(size_t)bi * D + d];
                                dd += e * e;
                            }
                            rowdist[row] = dd;
                        }
                        labels[row] = bi;
                    }
                    rowv[r] = ch;
                }
            } else {
                T mx = -INFINITY;
                int am = 0;
                for (int k = s; k < K; k += 16)
                    if (wr[k] > mx) { mx = wr[k]; am = k; }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    const T om = __shfl_xor(mx, o, 64);
                    const int oa = __shfl_xor(am, o, 64);
                    if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
                }
                T se = 0;
                for (int k = s; k < K; k += 16) se += exp(wr[k] - mx);
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
                const T lpn = log(se) + mx;   // scipy.special.logsumexp
                for (int k = s; k < K; k += 16) {
                    const T rk = r < rows ? exp(wr[k] - lpn) : (T)0;
                    wr[k] = rk;
                    if (out_resp && r < rows) out_resp[(row0 + r) * K + k] = rk;
                }
                if (s == 0) {
                    rowv[r] = r < rows ? (double)lpn : 0.0;
                    if (r < rows) {
                        if (out_lpn) out_lpn[row0 + r] = lpn;
                        if (out_label) out_label[row0 + r] = am;
                    }
                }
            }
        }
        if (!cols) continue;
        __syncthreads();
        // ---- column phase
#pragma unroll
        for (int j = 0; j < GPJ; ++j) {
            const int p = tid + j * GB;
            if (p < KD) {
                const int k = p / D, d = p - k * D;
                T t1 = 0, t2 = 0;
                if (mode == M_LLOYD) {
                    for (int r = 0; r < GR; ++r)
                        if (lab[r] == k) t1 += xs[r * (D + 1) + d];
                } else {
                    for (int r = 0; r < GR; ++r) {
                        const T w = ws[r * K + k], v = xs[r * (D + 1) + d];
                        t1 += w * v;
                        t2 += w * (v * v);
                    }
                }
                acc1[j] += (double)t1;
                acc2[j] += (double)t2;
            }
        }
        if (tid < K) {
            T t = 0;
            if (mode == M_LLOYD) {
                for (int r = 0; r < GR; ++r) t += lab[r] == tid ? (T)1 : (T)0;
            } else {
                for (int r = 0; r < GR; ++r) t += ws[r * K + tid];
            }
            accn += (double)t;
        }
        if (tid == GB - 1)
            for (int r = 0; r < GR; ++r) accs += rowv[r];
    }
    if (!cols) return;
    const size_t W = pass_width(mode == M_LLOYD ? M_LLOYD : M_EM, K, D);
    double* pw = part + (size_t)blockIdx.x * W;
#pragma unroll
    for (int j = 0; j < GPJ; ++j) {
        const int p = tid + j * GB;
        if (p < KD) {
            pw[p] = acc1[j];
            if (mode != M_LLOYD) pw[KD + p] = acc2[j];
        }
    }
    const size_t off = (size_t)KD * (mode == M_LLOYD ? 1 : 2);
    if (tid < K) pw[off + tid] = accn;
    if (tid == GB - 1) pw[off + K] = accs;
}

// out[m] = sum_g part[g][m], g in order
__global__ void gmm_reduce_partials(const double* part, int G, size_t W, double* out) {
    const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= W) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * W + m];
    out[m] = s;
}

template <typename T> __device__ void block_argmax(double& v, long long& i, double* sv, long long* si) {
    // (value desc, index asc) over the 1024 threads of the block; result in every thread
    const int tid = threadIdx.x;
    sv[tid] = v;
    si[tid] = i;
    __syncthreads();
    for (int o = GB / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double ov = sv[tid + o];
            const long long oi = si[tid + o];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
        }
        __syncthreads();
    }
    v = sv[0];
    i = si[0];
    __syncthreads();
}

// New centers from the reduced Lloyd partials: empty-cluster relocation (each empty cluster takes the farthest point not yet taken),
// average, center shift.  status[0] = changed labels, status[1] = sum_k ||c_new - c_old||^2.
template <typename T>
__global__ void __launch_bounds__(GB) lloyd_finalize(const T* X, size_t n, int D, int K, const T* mean, const T* centers_old,
                                                     const int32_t* labels, const T* rowdist, double* red, T* centers_new,
                                                     double* status) {
    __shared__ double sv[GB];
    __shared__ long long si[GB];
    __shared__ long long taken[GMAX];
    __shared__ int empties[GMAX];
    __shared__ int nempty;
    const int tid = threadIdx.x;
    const int KD = K * D;
    double* sums = red;
    double* cnt = red + KD;
    if (tid == 0) {
        int e = 0;
        for (int k = 0; k < K; ++k)
            if (cnt[k] == 0.0) empties[e++] = k;
        nempty = e;
    }
    __syncthreads();
    for (int e = 0; e < nempty; ++e) {
        double bv = -1.0;
        long long bi = -1;
        for (size_t i = tid; i < n; i += GB) {
            const double v = (double)rowdist[i];
            if (v > bv || (v == bv && (long long)i < bi)) {
                bool used = false;
                for (int q = 0; q < e; ++q) used |= taken[q] == (long long)i;
                if (!used) { bv = v; bi = (long long)i; }
            }
        }
        block_argmax<T>(bv, bi, sv, si);
        if (e == 0 && bv <= 0.0) break;   // every point sits on its center: sklearn leaves the empty clusters alone
        const int kn = empties[e], ko = labels[bi];
        for (int d = tid; d < D; d += GB) {
            T x = X[(size_t)bi * D + d];
            if (mean) x = x - mean[d];
            sums[(size_t)ko * D + d] -= (double)x;
            sums[(size_t)kn * D + d] = (double)x;
        }
        __syncthreads();
        if (tid == 0) {
            taken[e] = bi;
            cnt[kn] = 1.0;
            cnt[ko] -= 1.0;
        }
        __syncthreads();
    }
    int am = 0;   // np.argmax(weight_in_clusters)
    for (int k = 1; k < K; ++k)
        if (cnt[k] > cnt[am]) am = k;
    for (int p = tid; p < KD; p += GB) {
        const int k = p / D, d = p - k * D;
        const int src = cnt[k] > 0.0 ? k : am;
        centers_new[p] = (T)(sums[(size_t)src * D + d] * (1.0 / cnt[src]));
    }
    __syncthreads();
    double sh = 0.0;
    for (int p = tid; p < KD; p += GB) {
        const double e = (double)centers_new[p] - (double)centers_old[p];
        sh += e * e;
    }
    sv[tid] = sh;
    __syncthreads();
    for (int o = GB / 2; o > 0; o >>= 1) {
        if (tid < o) sv[tid] += sv[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        status[0] = red[KD + K];
        status[1] = sv[0];
    }
}

// Derived arrays of a parameter block from w, means, pchol (precisions_cholesky_): what _estimate_log_gaussian_prob forms each call
template <typename T> __device__ void params_prepare_body(Params<T> P, int K, int D) {
    const int tid = threadIdx.x;
    for (int p = tid; p < K * D; p += blockDim.x) {
        const T pc = P.pchol[p];
        P.prec[p] = pc * pc;
        P.mp[p] = P.means[p] * P.prec[p];
    }
    __syncthreads();
    for (int k = tid; k < K; k += blockDim.x) {
        double ld = 0.0, s = 0.0;
        for (int d = 0; d < D; ++d) {
            const double m = (double)P.means[(size_t)k * D + d];
            ld += log((double)P.pchol[(size_t)k * D + d]);
            s += m * m * (double)P.prec[(size_t)k * D + d];
        }
        P.logdet[k] = (T)ld;
        P.smp[k] = (T)s;
        P.logw[k] = log(P.w[k]);
    }
}

template <typename T> __global__ void gmm_params_prepare(void* pblock, int K, int D) { params_prepare_body<T>(Params<T>(pblock, K, D), K, D); }

// _estimate_gaussian_parameters (diag) from the reduced EM partials, then _m_step's normalisation (init = 0) or _initialize's
// weights / n_samples (init = 1); lb_out = mean log_prob_norm of the E-step that produced the partials (EM only).
template <typename T>
__global__ void __launch_bounds__(GB) gmm_mstep_finalize(const double* red, size_t n, int K, int D, double reg_covar, int init,
                                                         void* pblock, double* lb_out) {
    __shared__ double nks[GMAX];
    __shared__ double tot;
    Params<T> P(pblock, K, D);
    const int tid = threadIdx.x;
    const int KD = K * D;
    const double eps10 = 10.0 * (sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16);
    if (tid < K) nks[tid] = (double)(T)red[2 * KD + tid] + eps10;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += nks[k];
        tot = s;
        if (!init && lb_out) *lb_out = red[2 * KD + K] / (double)n;
    }
    __syncthreads();
    for (int p = tid; p < KD; p += GB) {
        const int k = p / D;
        const double nk = nks[k];
        const double m = red[p] / nk;
        const double cov = red[KD + p] / nk - 2.0 * (m * (red[p] / nk)) + m * m + reg_covar;
        P.means[p] = (T)m;
        P.covars[p] = (T)cov;
        P.pchol[p] = (T)1 / sqrt((T)cov);
    }
    if (tid < K) P.w[tid] = (T)(init ? nks[tid] / (double)n : nks[tid] / tot);
    __syncthreads();
    params_prepare_body<T>(P, K, D);
}

// ---- k-means++ (_kmeans_plusplus) --------------------------------------------------------------------------------------------
// Distances ||x||^2 - 2 x.c + ||c||^2 clipped at 0: norms in T (row_norms), the product in f64 (scikit-learn's float32 path upcasts
// it; float64 is float64 throughout).  closest_dist_sq and the candidate potentials are rounded to T as scikit-learn keeps them,
// and stored as f64.  Step s of the seeding writes buffer s % 2:
//   dist[c][n]   min(closest, d(x, cand_c)) of candidate c      csum[c][nch]   its per-chunk sums
//   best         index of the chosen candidate of the step      pot            its potential
// and step s+1 reads closest as buffer (s-1) % 2 row best.
struct KppState {
    double* dist[2];
    double* csum[2];
    int64_t* cand;
    int32_t* best;
    double* pot;
};

template <typename T>
__global__ void __launch_bounds__(KPP_R) kpp_dist(const T* __restrict__ X, size_t n, int D, const T* mean, const int64_t* cand,
                                                 int64_t first, int C, const double* prev,
                                                 const int32_t* best, double* dist, double* csum, size_t nch) {
    __shared__ double cs[KPP_LMAX * GMAX];
    __shared__ T cnorm[KPP_LMAX];
    __shared__ double red[KPP_R];
    const int tid = threadIdx.x;
    for (int i = tid; i < C * D; i += KPP_R) {
        const int c = i / D, d = i - c * D;
        const int64_t id = cand ? cand[c] : first;
        T v = X[(size_t)id * D + d];
        if (mean) v = v - mean[d];
        cs[i] = (double)v;
    }
    __syncthreads();
    if (tid < C) {
        T s = 0;
        for (int d = 0; d < D; ++d) {
            const T v = (T)cs[tid * D + d];
            s += v * v;
        }
        cnorm[tid] = s;
    }
    __syncthreads();
    const size_t row = (size_t)blockIdx.x * KPP_R + tid;
    double dots[KPP_LMAX];
#pragma unroll
    for (int c = 0; c < KPP_LMAX; ++c) dots[c] = 0.0;
    T xn = 0;
    if (row < n) {
        const T* xr = X + row * D;
        for (int d = 0; d < D; ++d) {
            T v = xr[d];
            if (mean) v = v - mean[d];
            xn += v * v;
            const double vd = (double)v;
#pragma unroll
            for (int c = 0; c < KPP_LMAX; ++c)
                if (c < C) dots[c] += vd * cs[c * D + d];
        }
    }
    const double closest = (prev && row < n) ? prev[(size_t)(*best) * n + row] : INFINITY;
    for (int c = 0; c < C; ++c) {
        double v = 0.0;
        if (row < n) {
            double dd = -2.0 * dots[c];
            dd += (double)xn;
            dd += (double)cnorm[c];
            dd = dd > 0.0 ? dd : 0.0;
            dd = (double)(T)dd;   // scikit-learn's distances (and closest_dist_sq) are in the dtype of X
            v = dd < closest ? dd : closest;
            dist[(size_t)c * n + row] = v;
        }
        red[tid] = v;
        __syncthreads();
        for (int o = KPP_R / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) csum[(size_t)c * nch + blockIdx.x] = red[0];
        __syncthreads();
    }
}

// np.searchsorted(cumsum(closest_dist_sq), u * current_pot) for the L trials of one step, clipped to n - 1
__global__ void __launch_bounds__(GB) kpp_search(const double* closest_all, const double* csum_all, const int32_t* best, size_t n,
                                                 size_t nch, const double* pot, const double* u, int L, int64_t* cand) {
    __shared__ double seg[GB];
    const int tid = threadIdx.x;
    const double* closest = closest_all + (size_t)(*best) * n;
    const double* csum = csum_all + (size_t)(*best) * nch;
    const size_t per = (nch + GB - 1) / GB;
    {
        double s = 0.0;
        for (size_t c = tid * per; c < std::min(nch, (size_t)(tid + 1) * per); ++c) s += csum[c];
        seg[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {   // inclusive prefix of the segment totals
        double s = 0.0;
        for (int i = 0; i < GB; ++i) { s += seg[i]; seg[i] = s; }
    }
    __syncthreads();
    if (tid < L) {
        const double v = u[tid] * (*pot);
        int sg = 0;
        while (sg < GB - 1 && seg[sg] < v) ++sg;
        double run = sg ? seg[sg - 1] : 0.0;
        int64_t idx = (int64_t)n - 1;   // v beyond the total (rounding): the last row, as np.clip does
        bool found = false;
        for (size_t c = (size_t)sg * per; c < nch && !found; ++c) {
            if (run + csum[c] < v) { run += csum[c]; continue; }
            for (size_t i = c * KPP_R; i < std::min(n, (c + 1) * KPP_R); ++i) {
                run += closest[i];
                if (run >= v) { idx = (int64_t)i; found = true; break; }
            }
        }
        cand[tid] = idx;
    }
}

// best candidate of the step (np.argmin of the potentials), the chosen center row (T, centred like X) and its one-hot label
template <typename T>
__global__ void __launch_bounds__(KPP_R) kpp_pick(const T* X, int D, const T* mean, const int64_t* cand, int64_t first, int C,
                                                 const double* csum, size_t nch, int step, int32_t* best, double* pot,
                                                 int64_t* indices, T* centers, int32_t* labels) {
    __shared__ double red[KPP_R];
    __shared__ int sbest;
    const int tid = threadIdx.x;
    double bp = INFINITY;
    int bc = 0;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (size_t i = tid; i < nch; i += KPP_R) s += csum[(size_t)c * nch + i];
        red[tid] = s;
        __syncthreads();
        for (int o = KPP_R / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        const double pc = (double)(T)red[0];   // candidates_pot in the dtype of X
        if (pc < bp) { bp = pc; bc = c; }
        __syncthreads();
    }
    if (tid == 0) {
        sbest = bc;
        *best = bc;
        *pot = bp;
        const int64_t id = cand ? cand[bc] : first;
        indices[step] = id;
        if (labels) labels[id] = step;
    }
    __syncthreads();
    const int64_t id = cand ? cand[sbest] : first;
    for (int d = tid; d < D; d += KPP_R) {
        T v = X[(size_t)id * D + d];
        if (mean) v = v - mean[d];
        centers[(size_t)step * D + d] = v;
    }
}

// column sums of (X - shift) and (X - shift)^2, f64 partials per workgroup
template <typename T>
__global__ void __launch_bounds__(256) colstats_partial(const T* X, size_t n, int D, const double* shift, double* part) {
    const int tid = threadIdx.x;
    for (int d = tid; d < D; d += 256) {
        double s1 = 0.0, s2 = 0.0;
        const double sh = shift ? shift[d] : 0.0;
        for (size_t r = blockIdx.x; r < n; r += gridDim.x) {
            const double v = (double)X[r * D + d] - sh;
            s1 += v;
            s2 += v * v;
        }
        part[(size_t)blockIdx.x * 2 * D + d] = s1;
        part[(size_t)blockIdx.x * 2 * D + D + d] = s2;
    }
}

size_t kpp_chunks(size_t n) { return (n + KPP_R - 1) / KPP_R; }

template <typename T> int launch_tile_pass(const T* X, size_t n, int D, int K, int mode, const T* mean, const T* centers,
                                           const void* pblock, int32_t* labels, T* rowdist, T* out_lpn, T* out_resp,
                                           int32_t* out_label, double* part, hipStream_t s) {
    const size_t lds = tile_lds(D, K, sizeof(T));
    if (int e = cpg_allow_big_lds((const void*)gmm_tile_pass<T>, (int)lds)) return e;
    hipLaunchKernelGGL(gmm_tile_pass<T>, dim3(pass_grid(n)), dim3(GB), lds, s, X, n, D, K, mode, mean, centers, pblock, labels,
                       rowdist, out_lpn, out_resp, out_label, part);
    CPG_LAUNCH_CHECK();
    return 0;
}

int launch_reduce(const double* part, int G, size_t W, double* out, hipStream_t s) {
    hipLaunchKernelGGL(gmm_reduce_partials, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, part, G, W, out);
    CPG_LAUNCH_CHECK();
    return 0;
}

bool shape_ok(size_t n, int D, int K, int dbytes) {
    return n > 0 && D > 0 && D <= GMAX && K > 0 && K <= GMAX && (dbytes == 4 || dbytes == 8) && n <= (size_t)1 << 40;
}

}  // namespace

CPG_EXPORT size_t cpg_gmm_workspace(size_t n, int D, int K) {
    if (n == 0 || D <= 0 || K <= 0) return 0;
    const size_t W = pass_width(M_EM, K, D);
    return ((size_t)GG + 1) * W * sizeof(double) + 2 * (size_t)GG * GMAX * sizeof(double);
}

CPG_EXPORT size_t cpg_gmm_params_elems(int D, int K) { return (size_t)K * (4 + 5 * (size_t)D); }

CPG_EXPORT int cpg_gmm_colstats(const void* X, size_t n, int D, int dbytes, const double* shift, double* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    CPG_CHECK_ARG(X && out && workspace && shape_ok(n, D, 1, dbytes));
    const int G = (int)std::min<size_t>(GG, n);
    CPG_CHECK_ARG(workspace_bytes >= (size_t)G * 2 * D * sizeof(double));
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (dbytes == 4) hipLaunchKernelGGL(colstats_partial<float>, dim3(G), dim3(256), 0, s, (const float*)X, n, D, shift, part);
    else hipLaunchKernelGGL(colstats_partial<double>, dim3(G), dim3(256), 0, s, (const double*)X, n, D, shift, part);
    CPG_LAUNCH_CHECK();
    return launch_reduce(part, G, 2 * (size_t)D, out, s);
}

CPG_EXPORT size_t cpg_kmeans_pp_workspace(size_t n, int n_trials) {
    if (n == 0 || n_trials <= 0) return 0;
    const size_t L = (size_t)n_trials, nch = kpp_chunks(n);
    return 2 * L * (n + nch) * sizeof(double) + L * sizeof(int64_t) + 2 * sizeof(double) + 64;
}

CPG_EXPORT int cpg_kmeans_pp(const void* X, size_t n, int D, int dbytes, const void* mean, int64_t first, const double* uniforms,
                             int K, int n_trials, int64_t* indices, void* centers, int32_t* labels, void* workspace,
                             size_t workspace_bytes, void* stream) {
    CPG_CHECK_ARG(X && indices && centers && workspace && shape_ok(n, D, 1, dbytes) && K > 0 && (size_t)K <= n);
    CPG_CHECK_ARG(n_trials > 0 && n_trials <= KPP_LMAX && first >= 0 && (size_t)first < n && (K == 1 || uniforms));
    CPG_CHECK_ARG(workspace_bytes >= cpg_kmeans_pp_workspace(n, n_trials));
    hipStream_t s = (hipStream_t)stream;
    const size_t L = n_trials, nch = kpp_chunks(n);
    char* w = (char*)workspace;
    KppState st;
    for (int b = 0; b < 2; ++b) { st.dist[b] = (double*)w; w += L * n * sizeof(double); }
    for (int b = 0; b < 2; ++b) { st.csum[b] = (double*)w; w += L * nch * sizeof(double); }
    st.pot = (double*)w; w += 2 * sizeof(double);
    st.cand = (int64_t*)w; w += L * sizeof(int64_t);
    st.best = (int32_t*)w;
    for (int c = 0; c < K; ++c) {
        const int cur = c & 1, prv = cur ^ 1;
        const int C = c == 0 ? 1 : n_trials;
        const int64_t* cand = c == 0 ? nullptr : st.cand;
        if (c > 0) {
            hipLaunchKernelGGL(kpp_search, dim3(1), dim3(GB), 0, s, st.dist[prv], st.csum[prv], st.best, n, nch, st.pot,
                               uniforms + (size_t)(c - 1) * n_trials, n_trials, st.cand);
            CPG_LAUNCH_CHECK();
        }
        const double* prev = c == 0 ? nullptr : st.dist[prv];
        if (dbytes == 4) {
            hipLaunchKernelGGL(kpp_dist<float>, dim3((unsigned)nch), dim3(KPP_R), 0, s, (const float*)X, n, D, (const float*)mean,
                               cand, first, C, prev, st.best, st.dist[cur], st.csum[cur], nch);
            CPG_LAUNCH_CHECK();
            hipLaunchKernelGGL(kpp_pick<float>, dim3(1), dim3(KPP_R), 0, s, (const float*)X, D, (const float*)mean, cand, first, C,
                               st.csum[cur], nch, c, st.best, st.pot, indices, (float*)centers, labels);
        } else {
            hipLaunchKernelGGL(kpp_dist<double>, dim3((unsigned)nch), dim3(KPP_R), 0, s, (const double*)X, n, D,
                               (const double*)mean, cand, first, C, prev, st.best, st.dist[cur], st.csum[cur], nch);
            CPG_LAUNCH_CHECK();
            hipLaunchKernelGGL(kpp_pick<double>, dim3(1), dim3(KPP_R), 0, s, (const double*)X, D, (const double*)mean, cand, first,
                               C, st.csum[cur], nch, c, st.best, st.pot, indices, (double*)centers, labels);
        }
        CPG_LAUNCH_CHECK();
    }
    return 0;
}

CPG_EXPORT int cpg_kmeans_lloyd_step(const void* X, size_t n, int D, int K, int dbytes, const void* mean, const void* centers,
                                     void* centers_new, int32_t* labels, void* rowdist, double* status, int update,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    CPG_CHECK_ARG(X && centers && labels && shape_ok(n, D, K, dbytes));
    CPG_CHECK_ARG(!update || (centers_new && rowdist && status && workspace && workspace_bytes >= cpg_gmm_workspace(n, D, K)));
    hipStream_t s = (hipStream_t)stream;
    const int G = pass_grid(n);
    const size_t W = pass_width(M_LLOYD, K, D);
    double* part = (double*)workspace;
    double* red = part + (size_t)GG * W;
    const int mode = update ? M_LLOYD : M_LABEL;
    int e = dbytes == 4 ? launch_tile_pass<float>((const float*)X, n, D, K, mode, (const float*)mean, (const float*)centers,
                                                  nullptr, labels, (float*)rowdist, nullptr, nullptr, nullptr, part, s)
                        : launch_tile_pass<double>((const double*)X, n, D, K, mode, (const double*)mean, (const double*)centers,
                                                   nullptr, labels, (double*)rowdist, nullptr, nullptr, nullptr, part, s);
    if (e || !update) return e;
    if ((e = launch_reduce(part, G, W, red, s))) return e;
    if (dbytes == 4)
        hipLaunchKernelGGL(lloyd_finalize<float>, dim3(1), dim3(GB), 0, s, (const float*)X, n, D, K, (const float*)mean,
                           (const float*)centers, labels, (const float*)rowdist, red, (float*)centers_new, status);
    else
        hipLaunchKernelGGL(lloyd_finalize<double>, dim3(1), dim3(GB), 0, s, (const double*)X, n, D, K, (const double*)mean,
                           (const double*)centers, labels, (const double*)rowdist, red, (double*)centers_new, status);
    CPG_LAUNCH_CHECK();
    return 0;
}

CPG_EXPORT int cpg_gmm_params_prepare(void* params, int D, int K, int dbytes, void* stream) {
    CPG_CHECK_ARG(params && shape_ok(1, D, K, dbytes));
    if (dbytes == 4) hipLaunchKernelGGL(gmm_params_prepare<float>, dim3(1), dim3(GB), 0, (hipStream_t)stream, params, K, D);
    else hipLaunchKernelGGL(gmm_params_prepare<double>, dim3(1), dim3(GB), 0, (hipStream_t)stream, params, K, D);
    CPG_LAUNCH_CHECK();
    return 0;
}

CPG_EXPORT int cpg_gmm_em_step(const void* X, size_t n, int D, int K, int dbytes, const void* params, const int32_t* labels,
                               double reg_covar, void* params_out, double* lower_bound, void* workspace, size_t workspace_bytes,
                               void* stream) {
    CPG_CHECK_ARG(X && params_out && workspace && shape_ok(n, D, K, dbytes) && workspace_bytes >= cpg_gmm_workspace(n, D, K));
    CPG_CHECK_ARG((labels != nullptr) != (params != nullptr) && params != params_out);
    hipStream_t s = (hipStream_t)stream;
    const int G = pass_grid(n);
    const size_t W = pass_width(M_EM, K, D);
    double* part = (double*)workspace;
    double* red = part + (size_t)GG * W;
    const int mode = labels ? M_INIT : M_EM;
    int32_t* lab = const_cast<int32_t*>(labels);
    int e = dbytes == 4 ? launch_tile_pass<float>((const float*)X, n, D, K, mode, nullptr, nullptr, params, lab, nullptr, nullptr,
                                                  nullptr, nullptr, part, s)
                        : launch_tile_pass<double>((const double*)X, n, D, K, mode, nullptr, nullptr, params, lab, nullptr, nullptr,
                                                   nullptr, nullptr, part, s);
    if (e || (e = launch_reduce(part, G, W, red, s))) return e;
    if (dbytes == 4)
        hipLaunchKernelGGL(gmm_mstep_finalize<float>, dim3(1), dim3(GB), 0, s, red, n, K, D, reg_covar, labels ? 1 : 0, params_out,
                           lower_bound);
    else
        hipLaunchKernelGGL(gmm_mstep_finalize<double>, dim3(1), dim3(GB), 0, s, red, n, K, D, reg_covar, labels ? 1 : 0, params_out,
                           lower_bound);
    CPG_LAUNCH_CHECK();
    return 0;
}

CPG_EXPORT int cpg_gmm_score(const void* X, size_t n, int D, int K, int dbytes, const void* params, void* log_prob_norm,
                             void* resp, int32_t* label, void* stream) {
    CPG_CHECK_ARG(X && params && shape_ok(n, D, K, dbytes) && (log_prob_norm || resp || label));
    hipStream_t s = (hipStream_t)stream;
    return dbytes == 4 ? launch_tile_pass<float>((const float*)X, n, D, K, M_SCORE, nullptr, nullptr, params, nullptr, nullptr,
                                                 (float*)log_prob_norm, (float*)resp, label, nullptr, s)
                       : launch_tile_pass<double>((const double*)X, n, D, K, M_SCORE, nullptr, nullptr, params, nullptr, nullptr,
                                                  (double*)log_prob_norm, (double*)resp, label, nullptr, s);
}
