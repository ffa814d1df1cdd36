// The Infomax familiarity model on the device (include/dejavu.h: dv_infomax_*).  One layer of weights W, double[M][N], trained once
// over the route's views (Baddeley, Graham, Husbands & Philippides 2012); a view's unfamiliarity is d(x) = sum_i |(W x)_i|.  Per
// training view, with x = p/255 - mean(p/255) of the view's compared plane:
//
//     h = W x;   y = tanh(h);   u = h^T W;   W <- W + (eta/N) * (W - (y + h) u^T)
//
// Everything is double and every reduction has a fixed order (no floating-point atomics), so two runs give the same bits.
// The grid-wide dependencies (u needs all of h, the update needs all of u) are kernel boundaries on the context's stream:
//
//   k_im_prep     one workgroup per view: plane bytes -> x (the mean's sum: 256 strided partial sums, then a fixed tree in LDS)
//   k_im_gemv     h = W x, one wave per row (a lane's strided partial sum, then the xor butterfly): the first h of a chain only
//   k_im_upart    pass A: partial u over blocks of kImRowsPerBlock rows, a thread per column, rows in order
//   k_im_ureduce  u_j = the partials of column j, row blocks in order (N threads: a launch of its own, since every workgroup of the
//                 update needs all of u and re-summing the partials there would cost more than the launch)
//   k_im_update   pass B: one wave per row updates the row and, in the same sweep, dots the UPDATED row with the NEXT view's x --
//                 the next h.  Same loop, same operations and same order as k_im_gemv on the stored row, so a chain cut in two
//                 (dv_infomax_train_u8 called twice) carries the bits of the uncut one.  W: read twice, written once per view.
//   k_im_score    H = W X for up to 64 headings and d's partial sums in one pass over W on the f64 matrix cores
//                 (v_mfma_f64_16x16x4_f64): a workgroup of 8 waves owns 16 rows of W, the waves take the 16-column chunks of those rows
//                 round-robin, their accumulators are added in wave order through LDS, then |.| is summed over the 16 rows in order
//   k_im_dfinish  d_a = the row tiles' partial sums (one wave per heading: strided partial sums, then the butterfly)
//   k_im_score_cols  an ensemble's step (dv_infomax_*_batch): k_im_score's body over a grid of row tiles x blocks of 64 columns, the
//                 members' headings being one flat list of columns (member i owns [i A, (i + 1) A)); dpart is [row tiles][C padded to 64]
//   k_im_decide   one workgroup per member: each of its columns summed as k_im_dfinish sums it and negated, then the member's first
//                 maximum and, from k_sense_each's word per pose, its DV_RES_SENSE_ERROR flag
//   k_im_finite   is every weight finite? (a too-large learning rate makes the rule diverge)
//
// Weight banks (dv_ibank_*).  W is double[n_banks][M][N], bank b at W + b M N with no padding; n_banks is 1 after dv_infomax_begin, and
// every dv_infomax_* / dv_batch_infomax_* call works on bank 0 through the kernels above.  The R routes of a grid are R independent
// chains: k_im_gemv_banks, k_im_upart_banks, k_im_ureduce_banks and k_im_update_banks advance them in lockstep -- step s of a call is
// every bank's s-th view, in the three launches one chain's step takes, the bank being the grid's last dimension -- with the bodies of
// the single model's kernels (device functions), so bank b ends with the bits of its chain run alone.  k_im_score_cols_banks is
// k_im_score_cols over column blocks that never mix banks (a table of blocks from the host: the members sorted by bank),
// k_im_decide_banks maps the columns back to the caller's members, k_im_finite_banks has a flag word per bank.
//
// Network tables (dejavu_inet.inl).  A live table (c->inet_nets > 0) gives every bank an n_hidden, a learning rate, a W0 and a channel of
// its own: W, h and upart are then ragged, and the banked host paths below (ibank_train_device, ibank_batch, the banks' finite flags,
// weights and error messages) hand over to k_inet_*, which are this file's device functions on a per-bank descriptor.  The kernels of
// this file are launched only without a table, and the calls that assume the begin's shape behind bank 0 are refused while one is
// live (infomax_need_bank0).
//
// A heading's column of H does not depend on how many headings ride with it (an MFMA result element is its own dot product), which
// is what lets the agent's fused step and a plug-in call on one patch agree bit for bit.
namespace dv {

__device__ __forceinline__ double im_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// src: view v's compared plane is src[v * view_stride + offset + j * px_stride], j < N
__global__ __launch_bounds__(256) void k_im_prep(const unsigned char* __restrict__ src, long long view_stride, int px_stride, int offset, int N,
                                                 double* __restrict__ x) {
    __shared__ double red[256];
    const int tid = (int)threadIdx.x;
    const unsigned char* p = src + (size_t)blockIdx.x * (size_t)view_stride + offset;
    double* xo = x + (size_t)blockIdx.x * (size_t)N;
    double s = 0.0;
    for (int j = tid; j < N; j += 256) s += (double)p[(size_t)j * px_stride] / 255.0;
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    const double mean = red[0] / (double)N;
    for (int j = tid; j < N; j += 256) xo[j] = (double)p[(size_t)j * px_stride] / 255.0 - mean;
}

// The bodies of the training kernels as device functions, so that the banked kernels (below) run bank b's chain with the operations and
// the order of the single model's.  k_im_upart and k_im_ureduce are these functions and nothing else: they compile to the instructions
// they had.  k_im_gemv, k_im_update, k_im_finite and k_im_decide keep a text of their own beside the function that restates it: called
// through it they compiled to the same operations in another instruction order, and the single model's code is to stay as it was.
__device__ __forceinline__ void im_gemv_rows(const double* __restrict__ W, const double* __restrict__ x, int M, int N, double* __restrict__ h) {
    const int lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (row >= M) return;                                   // (whole waves leave: no workgroup barrier below)
    const double* w = W + (size_t)row * (size_t)N;
    double acc = 0.0;
    for (int j = lane; j < N; j += 64) acc = __builtin_fma(w[j], x[j], acc);
    acc = im_wave_sum(acc);
    if (lane == 0) h[row] = acc;
}

__global__ __launch_bounds__(256) void k_im_gemv(const double* __restrict__ W, const double* __restrict__ x, int M, int N, double* __restrict__ h) {
    const int lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (row >= M) return;                                   // (whole waves leave: no workgroup barrier below)
    const double* w = W + (size_t)row * (size_t)N;
    double acc = 0.0;
    for (int j = lane; j < N; j += 64) acc = __builtin_fma(w[j], x[j], acc);
    acc = im_wave_sum(acc);
    if (lane == 0) h[row] = acc;
}

static constexpr int kImRowsPerBlock = 64;

__device__ __forceinline__ void im_upart_cols(const double* W, const double* h, int M, int N, double* upart) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= N) return;
    const int i0 = (int)blockIdx.y * kImRowsPerBlock;
    const int i1 = i0 + kImRowsPerBlock < M ? i0 + kImRowsPerBlock : M;
    const double* w = W + (size_t)i0 * (size_t)N + j;
    double acc = 0.0;
#pragma unroll 8
    for (int i = i0; i < i1; ++i, w += N) acc = __builtin_fma(h[i], *w, acc);
    upart[(size_t)blockIdx.y * (size_t)N + j] = acc;
}

__global__ __launch_bounds__(256) void k_im_upart(const double* __restrict__ W, const double* __restrict__ h, int M, int N, double* __restrict__ upart) {
    im_upart_cols(W, h, M, N, upart);
}

__device__ __forceinline__ void im_ureduce_cols(const double* upart, int n_blocks, int N, double* u) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= N) return;
    double acc = 0.0;
    for (int b = 0; b < n_blocks; ++b) acc += upart[(size_t)b * (size_t)N + j];
    u[j] = acc;
}

__global__ __launch_bounds__(256) void k_im_ureduce(const double* __restrict__ upart, int n_blocks, int N, double* __restrict__ u) {
    im_ureduce_cols(upart, n_blocks, N, u);
}

// x_next == nullptr: the chain ends here (h_next is not written)
__device__ __forceinline__ void im_update_rows(double* __restrict__ W, const double* __restrict__ h, const double* __restrict__ u, int M, int N,
                                               double rate, const double* __restrict__ x_next, double* __restrict__ h_next) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (row >= M) return;
    double* w = W + (size_t)row * (size_t)N;
    const double hi = h[row];
    const double yh = tanh(hi) + hi;
    double acc = 0.0;
    if (x_next) {
        for (int j = lane; j < N; j += 64) {
            const double wo = w[j];
            const double wn = wo + rate * (wo - yh * u[j]);
            w[j] = wn;
            acc = __builtin_fma(wn, x_next[j], acc);
        }
        acc = im_wave_sum(acc);
        if (lane == 0) h_next[row] = acc;
    } else {
        for (int j = lane; j < N; j += 64) {
            const double wo = w[j];
            w[j] = wo + rate * (wo - yh * u[j]);
        }
    }
}

__global__ __launch_bounds__(256) void k_im_update(double* __restrict__ W, const double* __restrict__ h, const double* __restrict__ u, int M, int N,
                                                   double rate, const double* __restrict__ x_next, double* __restrict__ h_next) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (row >= M) return;
    double* w = W + (size_t)row * (size_t)N;
    const double hi = h[row];
    const double yh = tanh(hi) + hi;
    double acc = 0.0;
    if (x_next) {
        for (int j = lane; j < N; j += 64) {
            const double wo = w[j];
            const double wn = wo + rate * (wo - yh * u[j]);
            w[j] = wn;
            acc = __builtin_fma(wn, x_next[j], acc);
        }
        acc = im_wave_sum(acc);
        if (lane == 0) h_next[row] = acc;
    } else {
        for (int j = lane; j < N; j += 64) {
            const double wo = w[j];
            w[j] = wo + rate * (wo - yh * u[j]);
        }
    }
}

__device__ __forceinline__ bool im_any_not_finite(const double* __restrict__ W, long long n) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) bad |= !isfinite(W[i]);
    return bad;
}

__global__ __launch_bounds__(256) void k_im_finite(const double* __restrict__ W, long long n, int* __restrict__ flag) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) bad |= !isfinite(W[i]);
    if (bad) *flag = 1;                                     // (every writer stores the same word)
}

// ---- weight banks: training (dv_ibank_train_*) ----
// W: [banks][M][N]; h, u, upart: a copy per bank.  The grid's last dimension is the bank.  tab: the slab's chains -- tab[b] = the views of
// bank b in the slab, tab[banks + b] = where b's list of x vectors begins in idx; idx[...] = a view's place in xs.  Step s of the slab
// takes every bank's s-th view: a workgroup whose bank has none leaves as a whole (its wave-uniform test comes before any work).
__global__ __launch_bounds__(256) void k_im_gemv_banks(const double* __restrict__ W, const double* __restrict__ xs, int M, int N, double* __restrict__ h,
                                                       const int* __restrict__ tab, const int* __restrict__ idx) {
    const int b = (int)blockIdx.y;
    if (tab[b] < 1) return;
    im_gemv_rows(W + (size_t)b * (size_t)M * (size_t)N, xs + (size_t)idx[tab[gridDim.y + b]] * (size_t)N, M, N, h + (size_t)b * (size_t)M);
}

__global__ __launch_bounds__(256) void k_im_upart_banks(const double* __restrict__ W, const double* __restrict__ h, int M, int N,
                                                        double* __restrict__ upart, const int* __restrict__ tab, int s) {
    const int b = (int)blockIdx.z;
    if (s >= tab[b]) return;
    im_upart_cols(W + (size_t)b * (size_t)M * (size_t)N, h + (size_t)b * (size_t)M, M, N, upart + (size_t)b * (size_t)gridDim.y * (size_t)N);
}

__global__ __launch_bounds__(256) void k_im_ureduce_banks(const double* __restrict__ upart, int n_blocks, int N, double* __restrict__ u,
                                                          const int* __restrict__ tab, int s) {
    const int b = (int)blockIdx.y;
    if (s >= tab[b]) return;
    im_ureduce_cols(upart + (size_t)b * (size_t)n_blocks * (size_t)N, n_blocks, N, u + (size_t)b * (size_t)N);
}

__global__ __launch_bounds__(256) void k_im_update_banks(double* __restrict__ W, const double* __restrict__ h, const double* __restrict__ u, int M, int N,
                                                         double rate, const double* __restrict__ xs, double* __restrict__ h_next,
                                                         const int* __restrict__ tab, const int* __restrict__ idx, int s) {
    const int b = (int)blockIdx.y, len = tab[b];
    if (s >= len) return;
    const double* x_next = s + 1 < len ? xs + (size_t)idx[tab[gridDim.y + b] + s + 1] * (size_t)N : nullptr;
    im_update_rows(W + (size_t)b * (size_t)M * (size_t)N, h + (size_t)b * (size_t)M, u + (size_t)b * (size_t)N, M, N, rate, x_next,
                   h_next + (size_t)b * (size_t)M);
}

// flag: a word per bank (blockIdx.y)
__global__ __launch_bounds__(256) void k_im_finite_banks(const double* __restrict__ W, long long n, int* __restrict__ flag) {
    if (im_any_not_finite(W + (size_t)blockIdx.y * (size_t)n, n)) flag[blockIdx.y] = 1;
}

typedef double im_d4 __attribute__((ext_vector_type(4)));

// The 4 doubles base[k .. k+3] of one row (zeros where ok is false or past n).  VEC: n % 4 == 0 and k % 4 == 0, so the four are there
// together and 32-byte aligned.
template <bool VEC>
__device__ __forceinline__ im_d4 im_load4(const double* __restrict__ base, int k, int n, bool ok) {
    im_d4 v = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
        if (ok && k < n) v = *reinterpret_cast<const im_d4*>(base + k);
    } else if (ok) {
        if (k < n) v.x = base[k];
        if (k + 1 < n) v.y = base[k + 1];
        if (k + 2 < n) v.z = base[k + 2];
        if (k + 3 < n) v.w = base[k + 3];
    }
    return v;
}

static constexpr int kImScoreWaves = 8;
static constexpr int kImHeadings = 64;                       // headings of one pass over W

// HT: 16-heading tiles computed (the call's headings, rounded up).  X: [A][N], heading-major.  dpart: [row tiles][kImHeadings].
// Lane l = (r = l & 15, g = l >> 4) feeds row r of the workgroup's 16 rows of W as the MFMA's A operand and heading r of each tile as
// its B operand, element k = chunk * 16 + g * 4 + j in MFMA j of 4; accumulator register q of tile t is H[row g + 4 q][heading 16 t + r].
// sred: [16][HT * 16] doubles of LDS; dout: where the tile's HT * 16 partial sums go.
template <int HT, bool VEC>
__device__ __forceinline__ void im_score_tile(const double* __restrict__ W, const double* __restrict__ X, int M, int N, int A, int tile,
                                              double* __restrict__ sred, double* __restrict__ dout) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int row = tile * 16 + r;
    const bool row_ok = row < M;
    const double* wrow = W + (size_t)(row_ok ? row : 0) * (size_t)N;
    const double* xrow[HT];
    bool x_ok[HT];
    im_d4 acc[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        const int a = t * 16 + r;
        x_ok[t] = a < A;
        xrow[t] = X + (size_t)(x_ok[t] ? a : 0) * (size_t)N;
        acc[t] = im_d4{0.0, 0.0, 0.0, 0.0};
    }
    const int n_chunks = (N + 15) / 16;
    // two of the wave's chunks per trip (chunk c and c + 8: loaded together, used in that order; a chunk past the end loads zeros)
    for (int c = wave; c < n_chunks; c += 2 * kImScoreWaves) {   // (wave-uniform bounds: every lane runs every MFMA)
        const int k0 = c * 16 + g * 4, k1 = k0 + 16 * kImScoreWaves;
        const im_d4 wv0 = im_load4<VEC>(wrow, k0, N, row_ok);
        const im_d4 wv1 = im_load4<VEC>(wrow, k1, N, row_ok);
        im_d4 xv0[HT], xv1[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            xv0[t] = im_load4<VEC>(xrow[t], k0, N, x_ok[t]);
            xv1[t] = im_load4<VEC>(xrow[t], k1, N, x_ok[t]);
        }
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv0.x, xv0[t].x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv0.y, xv0[t].y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv0.z, xv0[t].z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv0.w, xv0[t].w, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv1.x, xv1[t].x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv1.y, xv1[t].y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv1.z, xv1[t].z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv1.w, xv1[t].w, acc[t], 0, 0, 0);
        }
    }
    // the waves' shares of the sum over k, added in wave order
    for (int w = 0; w < kImScoreWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < HT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    double* s = &sred[(g + 4 * q) * (HT * 16) + t * 16 + r];
                    *s = w == 0 ? acc[t][q] : *s + acc[t][q];
                }
            }
        }
        __syncthreads();
    }
    if (tid < HT * 16) {
        double s = 0.0;
        for (int rr = 0; rr < 16; ++rr) s += fabs(sred[rr * (HT * 16) + tid]);   // (rows past M hold zeros)
        dout[tid] = s;
    }
}

template <int HT, bool VEC>
__global__ __launch_bounds__(kImScoreWaves * 64) void k_im_score(const double* __restrict__ W, const double* __restrict__ X, int M, int N, int A,
                                                                 double* __restrict__ dpart) {
    __shared__ double sred[16 * HT * 16];
    im_score_tile<HT, VEC>(W, X, M, N, A, (int)blockIdx.x, sred, dpart + (size_t)blockIdx.x * kImHeadings);
}

// C columns (X: [C][N]) in blocks of kImHeadings: workgroup (x, y) takes row tile x of column block y with the body above, so a column
// has the sums k_im_score gives it however many ride with it.  dpart: [row tiles][cpad], cpad = the call's columns padded to 64; the
// last block computes only the 16-column tiles it needs.
template <bool VEC>
__global__ __launch_bounds__(kImScoreWaves * 64) void k_im_score_cols(const double* __restrict__ W, const double* __restrict__ X, int M, int N, int C,
                                                                      long long cpad, double* __restrict__ dpart) {
    __shared__ double sred[16 * kImHeadings];
    const int c0 = (int)blockIdx.y * kImHeadings;
    const int nc = C - c0 < kImHeadings ? C - c0 : kImHeadings;          // (uniform over the workgroup)
    const double* Xb = X + (size_t)c0 * (size_t)N;
    double* dout = dpart + (size_t)blockIdx.x * (size_t)cpad + c0;
    if (nc <= 16) im_score_tile<1, VEC>(W, Xb, M, N, nc, (int)blockIdx.x, sred, dout);
    else if (nc <= 32) im_score_tile<2, VEC>(W, Xb, M, N, nc, (int)blockIdx.x, sred, dout);
    else im_score_tile<4, VEC>(W, Xb, M, N, nc, (int)blockIdx.x, sred, dout);
}

// The banked step's form (dv_ibank_step_u8 / dv_ibank_sense_step).  The members come sorted by bank, so a bank's columns are one run of
// X; the host cuts every run into blocks of at most 64 columns, so no block mixes banks: blocks[blockIdx.y] = {bank, first column of X
// (counted from the call's first), columns, first column of dpart}.  In dpart every bank's run begins at a multiple of 64 and is padded
// to one, so the zeros a block writes past its last column (im_score_tile fills whole 16-column tiles) land in padding.
struct ImBlock { int bank, x0, nc, d0; };

template <bool VEC>
__global__ __launch_bounds__(kImScoreWaves * 64) void k_im_score_cols_banks(const double* __restrict__ W, const double* __restrict__ X, int M, int N,
                                                                            const ImBlock* __restrict__ blocks, int x_first, long long cpad,
                                                                            double* __restrict__ dpart) {
    __shared__ double sred[16 * kImHeadings];
    const ImBlock bk = blocks[blockIdx.y];                               // (uniform over the workgroup)
    const double* Wb = W + (size_t)bk.bank * (size_t)M * (size_t)N;
    const double* Xb = X + (size_t)(bk.x0 - x_first) * (size_t)N;
    double* dout = dpart + (size_t)blockIdx.x * (size_t)cpad + bk.d0;
    if (bk.nc <= 16) im_score_tile<1, VEC>(Wb, Xb, M, N, bk.nc, (int)blockIdx.x, sred, dout);
    else if (bk.nc <= 32) im_score_tile<2, VEC>(Wb, Xb, M, N, bk.nc, (int)blockIdx.x, sred, dout);
    else im_score_tile<4, VEC>(Wb, Xb, M, N, bk.nc, (int)blockIdx.x, sred, dout);
}

// one wave per heading
__global__ __launch_bounds__(64) void k_im_dfinish(const double* __restrict__ dpart, int n_tiles, double* __restrict__ d) {
    const int lane = (int)threadIdx.x;
    double s = 0.0;
    for (int t = lane; t < n_tiles; t += 64) s += dpart[(size_t)t * kImHeadings + blockIdx.x];
    s = im_wave_sum(s);
    if (lane == 0) d[blockIdx.x] = s;
}

// One workgroup of 4 waves per member i of A columns.  fam[i][a] = -(column i A + a summed over the row tiles in k_im_dfinish's order);
// best[i] = the first maximum of the row; perr (nullptr: the patches were uploaded) holds k_sense_each's word per column: a member
// with one set gets best -1 and kResSenseError, its row is whatever its stale patches scored.
// The body: the member's A columns begin at dcol0 in dpart, at col0 in perr; row, best and flags are the member's own.
__device__ __forceinline__ void im_decide_member(const double* __restrict__ dpart, int n_tiles, long long cpad, int A,
                                                 const int* __restrict__ perr, size_t dcol0, size_t col0, double* __restrict__ row,
                                                 int* __restrict__ best, unsigned* __restrict__ flags) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    for (int a = wave; a < A; a += 4) {
        double s = 0.0;
        for (int t = lane; t < n_tiles; t += 64) s += dpart[(size_t)t * (size_t)cpad + dcol0 + a];
        s = im_wave_sum(s);
        if (lane == 0) row[a] = -s;
    }
    __syncthreads();
    if (wave != 0) return;
    // a lane's first maximum over its columns in rising order, then the lanes' maxima: the larger value, the lower column of equals
    double bv = 0.0;
    int bi = -1, bad = 0;
    for (int a = lane; a < A; a += 64) {
        const double v = row[a];
        if (bi < 0 || v > bv) { bv = v; bi = a; }
        if (perr) bad |= perr[col0 + a];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        bad |= __shfl_xor(bad, off);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        *best = bad ? -1 : bi;
        *flags = bad ? kResSenseError : 0u;
    }
}

__global__ __launch_bounds__(256) void k_im_decide(const double* __restrict__ dpart, int n_tiles, long long cpad, int A, const int* __restrict__ perr,
                                                   double* __restrict__ fam, int* __restrict__ best, unsigned* __restrict__ flags) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const size_t col0 = (size_t)blockIdx.x * (size_t)A;
    double* row = fam + col0;
    for (int a = wave; a < A; a += 4) {
        double s = 0.0;
        for (int t = lane; t < n_tiles; t += 64) s += dpart[(size_t)t * (size_t)cpad + col0 + a];
        s = im_wave_sum(s);
        if (lane == 0) row[a] = -s;
    }
    __syncthreads();
    if (wave != 0) return;
    // a lane's first maximum over its columns in rising order, then the lanes' maxima: the larger value, the lower column of equals
    double bv = 0.0;
    int bi = -1, bad = 0;
    for (int a = lane; a < A; a += 64) {
        const double v = row[a];
        if (bi < 0 || v > bv) { bv = v; bi = a; }
        if (perr) bad |= perr[col0 + a];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        bad |= __shfl_xor(bad, off);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        best[blockIdx.x] = bad ? -1 : bi;
        flags[blockIdx.x] = bad ? kResSenseError : 0u;
    }
}

// The banked step's form: member blockIdx.x of the CALLER's order; mem[2 i] = where its columns begin in dpart, mem[2 i + 1] = in X and
// perr (bank order).  fam, best and flags are in the caller's order.
__global__ __launch_bounds__(256) void k_im_decide_banks(const double* __restrict__ dpart, int n_tiles, long long cpad, int A,
                                                         const int* __restrict__ perr, const int* __restrict__ mem, double* __restrict__ fam,
                                                         int* __restrict__ best, unsigned* __restrict__ flags) {
    im_decide_member(dpart, n_tiles, cpad, A, perr, (size_t)mem[2 * blockIdx.x], (size_t)mem[2 * blockIdx.x + 1],
                     fam + (size_t)blockIdx.x * (size_t)A, best + blockIdx.x, flags + blockIdx.x);
}

}  // namespace dv

static constexpr long long kImMaxPixels = 1 << 20;            // N of a view
static constexpr size_t kImStageBytes = 64u << 20;            // x vectors and uploaded planes are staged in slabs of at most this

// Network tables (dejavu_inet.inl, which follows this file): a live one (c->inet_nets > 0) gives every bank a shape, a rate and a channel
// of its own, and the banked calls below go through its kernels.
static void inet_drop(dv_ctx* c);
static int inet_prep(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, int by_channel, long long n, double* x,
                     const int* d_bank_of, long long col0, int per);
static int inet_train_slab(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, long long nb, const int* d_tab, const int* d_idx,
                           const int* d_bank_of, int steps);
static int inet_finite(dv_ctx* c);
static int inet_score(dv_ctx* c, const dv::ImBlock* d_blocks, size_t nk, long long c0, long long cpad);
static int inet_decide(dv_ctx* c, int n_agents, long long cpad, int A, const int* perr, const int* d_mem, const int* d_bank_of, double* d_fam, int* d_best,
                       unsigned* d_flags);

static void infomax_free(dv_ctx* c) {
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->im_W); F(c->im_h[0]); F(c->im_h[1]); F(c->im_u); F(c->im_upart); F(c->im_xs); F(c->im_sx); F(c->im_dpart); F(c->im_d); F(c->im_flag);
    F(c->im_bx); F(c->im_bdpart); F(c->im_res.dev); F(c->im_perr);
    c->im_bx_cap = c->im_bdpart_cap = c->im_res.cap = c->im_perr_cap = 0;
    c->im_M = c->im_N = c->im_hh = c->im_ww = 0;
    c->im_xs_cap = 0;
    F(c->im_kh[0]); F(c->im_kh[1]); F(c->im_ku); F(c->im_kupart);
    table_free(c->im_ktab);
    inet_drop(c);
    c->im_w0.clear();
    c->im_banks = 1;
    c->im_views.assign(1, 0);
    c->im_finite.assign(1, 1);
}

static int infomax_need(dv_ctx* c, const char* who) {
    if (!c->im_W) return fail(c, DV_ERR_STATE, "%s: no Infomax model (dv_infomax_begin first)", who);
    return DV_OK;
}

// The calls that assume the begin's shape behind bank 0 (dv_infomax_*, dv_batch_infomax_*): refused while a network table is live.
static int infomax_need_bank0(dv_ctx* c, const char* who) {
    int rc = infomax_need(c, who);
    if (rc) return rc;
    if (c->inet_nets)
        return fail(c, DV_ERR_STATE, "%s: a network table is live, and bank 0 is no longer the model dv_infomax_begin made (dv_inet_clear first, or the dv_ibank_ call)", who);
    return DV_OK;
}

// Where bank `bank` lies in im_W, in doubles, and how many it holds: M N of the model, or under a network table of the bank's own network.
static void ibank_span(const dv_ctx* c, int bank, size_t& off, size_t& len) {
    const size_t N = (size_t)c->im_N;
    if (c->inet_nets) { off = c->inet_row0[(size_t)bank] * N; len = (size_t)c->inet_M[(size_t)c->inet_of_bank[(size_t)bank]] * N; }
    else { len = (size_t)c->im_M * N; off = (size_t)bank * len; }
}

// The learning rate bank `bank` is trained with: the model's, or under a network table its own network's.
static double ibank_eta(const dv_ctx* c, int bank) {
    return c->inet_nets ? c->inet_eta[(size_t)c->inet_of_bank[(size_t)bank]] : c->im_eta;
}

// Sets im_finite[bank] from the bank's weights as they stand (synchronises the stream).
static int infomax_check_finite(dv_ctx* c, int bank = 0) {
    size_t off, len;
    ibank_span(c, bank, off, len);
    const long long n = (long long)len;
    HIP_TRY(c, hipMemsetAsync(c->im_flag + bank, 0, sizeof(int), c->stream));
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_im_finite, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, c->stream, c->im_W + off, n,
                       c->im_flag + bank);
    HIP_TRY(c, hipGetLastError());
    int bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, c->im_flag + bank, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->im_finite[(size_t)bank] = bad == 0;
    return DV_OK;
}

static int infomax_not_finite(dv_ctx* c, const char* who) {
    return fail(c, DV_ERR_STATE, "%s: the weights are not finite (learning_rate %g is too large for these views: the rule diverged)", who,
                c->im_eta);
}

// The x vectors of a training slab: at most kImStageBytes of them, made at first use.
static int infomax_stage_x(dv_ctx* c) {
    if (c->im_xs) return DV_OK;
    size_t cap = kImStageBytes / ((size_t)c->im_N * sizeof(double));
    if (cap < 1) cap = 1;
    HIP_TRY(c, hipMalloc((void**)&c->im_xs, cap * (size_t)c->im_N * sizeof(double)));
    c->im_xs_cap = cap;
    return DV_OK;
}

// Enqueue the training chain over n views resident on the device (layout as k_im_prep's src).
static int infomax_train_device(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, int offset, int64_t n) {
    const int M = c->im_M, N = c->im_N;
    int rc = infomax_stage_x(c);
    if (rc) return rc;
    const double rate = c->im_eta / (double)N;
    const unsigned row_blocks = (unsigned)((M + 3) / 4), col_blocks = (unsigned)((N + 255) / 256);
    const int n_rb = (M + kImRowsPerBlock - 1) / kImRowsPerBlock;
    int cur = 0;
    for (int64_t b0 = 0; b0 < n; b0 += (int64_t)c->im_xs_cap) {
        const int64_t nb = n - b0 < (int64_t)c->im_xs_cap ? n - b0 : (int64_t)c->im_xs_cap;
        hipLaunchKernelGGL(k_im_prep, dim3((unsigned)nb), dim3(256), 0, c->stream, d_src + (size_t)b0 * (size_t)view_stride, view_stride, px_stride,
                           offset, N, c->im_xs);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(k_im_gemv, dim3(row_blocks), dim3(256), 0, c->stream, c->im_W, c->im_xs, M, N, c->im_h[cur]);
        HIP_TRY(c, hipGetLastError());
        for (int64_t v = 0; v < nb; ++v) {
            hipLaunchKernelGGL(k_im_upart, dim3(col_blocks, (unsigned)n_rb), dim3(256), 0, c->stream, c->im_W, c->im_h[cur], M, N, c->im_upart);
            hipLaunchKernelGGL(k_im_ureduce, dim3(col_blocks), dim3(256), 0, c->stream, c->im_upart, n_rb, N, c->im_u);
            const double* x_next = v + 1 < nb ? c->im_xs + (size_t)(v + 1) * (size_t)N : nullptr;
            hipLaunchKernelGGL(k_im_update, dim3(row_blocks), dim3(256), 0, c->stream, c->im_W, c->im_h[cur], c->im_u, M, N, rate, x_next,
                               c->im_h[cur ^ 1]);
            HIP_TRY(c, hipGetLastError());
            cur ^= 1;
        }
    }
    c->im_views[0] += n;
    return DV_OK;
}

template <int HT>
static void infomax_launch_score(dv_ctx* c, int n) {
    const unsigned tiles = (unsigned)((c->im_M + 15) / 16);
    if (c->im_N % 4 == 0)
        hipLaunchKernelGGL((k_im_score<HT, true>), dim3(tiles), dim3(kImScoreWaves * 64), 0, c->stream, c->im_W, c->im_sx, c->im_M, c->im_N, n, c->im_dpart);
    else
        hipLaunchKernelGGL((k_im_score<HT, false>), dim3(tiles), dim3(kImScoreWaves * 64), 0, c->stream, c->im_W, c->im_sx, c->im_M, c->im_N, n, c->im_dpart);
}

// Enqueue: x of the n <= 64 views at d_src, d of each, and the copy of the n values to `out` (the caller synchronises).
static int infomax_score_device(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, int offset, int n, double* out) {
    hipLaunchKernelGGL(k_im_prep, dim3((unsigned)n), dim3(256), 0, c->stream, d_src, view_stride, px_stride, offset, c->im_N, c->im_sx);
    HIP_TRY(c, hipGetLastError());
    if (n <= 16) infomax_launch_score<1>(c, n);
    else if (n <= 32) infomax_launch_score<2>(c, n);
    else infomax_launch_score<4>(c, n);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_im_dfinish, dim3((unsigned)n), dim3(64), 0, c->stream, c->im_dpart, (c->im_M + 15) / 16, c->im_d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, c->im_d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return DV_OK;
}

extern "C" int dv_infomax_end(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    infomax_free(c);
    return DV_OK;
}

extern "C" int dv_infomax_begin(dv_ctx* c, int h, int w, int channel, int n_hidden, double learning_rate, const double* w0) {
    if (!c) return DV_ERR_INVALID;
    if (!w0) return fail(c, DV_ERR_INVALID, "dv_infomax_begin: the initial weights are NULL");
    if (h < 1 || w < 1 || (long long)h * w > kImMaxPixels) return fail(c, DV_ERR_INVALID, "dv_infomax_begin: views of %d x %d (1..%lld pixels)", h, w, kImMaxPixels);
    if (channel < 0 || channel > 2) return fail(c, DV_ERR_INVALID, "dv_infomax_begin: channel %d outside [0, 2]", channel);
    if (n_hidden < 1 || n_hidden > kImMaxPixels) return fail(c, DV_ERR_INVALID, "dv_infomax_begin: n_hidden %d outside [1, %lld]", n_hidden, kImMaxPixels);
    if (!(learning_rate > 0.0) || !std::isfinite(learning_rate)) return fail(c, DV_ERR_INVALID, "dv_infomax_begin: learning_rate %g must be positive", learning_rate);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    infomax_free(c);
    const int M = n_hidden, N = h * w;
    const size_t wbytes = (size_t)M * (size_t)N * sizeof(double);
    const size_t n_rb = (size_t)((M + kImRowsPerBlock - 1) / kImRowsPerBlock), tiles = (size_t)((M + 15) / 16);
    hipError_t e = hipMalloc((void**)&c->im_W, wbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_h[0], (size_t)M * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_h[1], (size_t)M * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_u, (size_t)N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_upart, n_rb * (size_t)N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_sx, (size_t)kImHeadings * (size_t)N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_dpart, tiles * kImHeadings * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_d, kImHeadings * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_flag, sizeof(int));
    if (e == hipSuccess) e = hipMemcpyAsync(c->im_W, w0, wbytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // `w0` is borrowed for this call only
    if (e != hipSuccess) {
        (void)hipGetLastError();
        infomax_free(c);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_infomax_begin: %d x %d weights (%zu bytes): %s", M, N, wbytes,
                    hipGetErrorString(e));
    }
    c->im_M = M; c->im_N = N; c->im_hh = h; c->im_ww = w; c->im_channel = channel; c->im_eta = learning_rate;
    c->im_w0.assign(w0, w0 + (size_t)M * (size_t)N);         // (dv_inet_clear returns bank 0 to it)
    return infomax_check_finite(c);
}

extern "C" int dv_infomax_train_u8(dv_ctx* c, const uint8_t* planes, int64_t n) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_infomax_train_u8");
    if (rc) return rc;
    if (!planes || n < 0) return fail(c, DV_ERR_INVALID, "dv_infomax_train_u8: planes is NULL or n < 0");
    if (!c->im_finite[0]) return infomax_not_finite(c, "dv_infomax_train_u8");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->im_N;
    size_t slab = kImStageBytes / N;
    if (slab < 1) slab = 1;
    if ((int64_t)slab > n) slab = (size_t)n;
    if (n > 0) { rc = ensure_sense_buffer(c, slab * N); if (rc) return rc; }
    for (int64_t v0 = 0; v0 < n; v0 += (int64_t)slab) {
        const int64_t ns = n - v0 < (int64_t)slab ? n - v0 : (int64_t)slab;
        HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)v0 * N, (size_t)ns * N, hipMemcpyHostToDevice, c->stream));
        rc = infomax_train_device(c, c->d_sense, (long long)N, 1, 0, ns);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // the slab is reused, `planes` is borrowed
    }
    rc = infomax_check_finite(c);
    if (rc) return rc;
    return c->im_finite[0] ? DV_OK : infomax_not_finite(c, "dv_infomax_train_u8");
}

extern "C" int dv_infomax_train_from_poses(dv_ctx* c, const double* x, const double* y, const double* angle, int64_t n, uint8_t* out_views) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_infomax_train_from_poses");
    if (rc) return rc;
    if (!x || !y || !angle || n < 1 || n > 0x7fffffff) return fail(c, DV_ERR_INVALID, "dv_infomax_train_from_poses: bad arguments");
    rc = sensor_fits(c, "dv_infomax_train_from_poses", c->im_hh, c->im_ww);
    if (rc) return rc;
    if (!c->im_finite[0]) return infomax_not_finite(c, "dv_infomax_train_from_poses");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * (size_t)c->im_N * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    rc = enqueue_sense(c, x, y, angle, n, c->d_sense);
    if (rc) return rc;
    if (out_views) HIP_TRY(c, hipMemcpyAsync(out_views, c->d_sense, bytes, hipMemcpyDeviceToHost, c->stream));
    rc = check_sense_error(c);
    if (rc) return rc;
    rc = infomax_train_device(c, c->d_sense, 3ll * c->im_N, 3, c->im_channel, n);
    if (rc) return rc;
    rc = infomax_check_finite(c);
    if (rc) return rc;
    return c->im_finite[0] ? DV_OK : infomax_not_finite(c, "dv_infomax_train_from_poses");
}

extern "C" int dv_infomax_score_u8(dv_ctx* c, const uint8_t* planes, int n, double* familiarity) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_infomax_score_u8");
    if (rc) return rc;
    if (!planes || !familiarity || n < 1) return fail(c, DV_ERR_INVALID, "dv_infomax_score_u8: NULL argument or n < 1");
    if (!c->im_finite[0]) return infomax_not_finite(c, "dv_infomax_score_u8");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->im_N;
    rc = ensure_sense_buffer(c, (size_t)kImHeadings * N * 3);                // (the size dv_infomax_sense_step asks for: one allocation for both)
    if (rc) return rc;
    for (int a0 = 0; a0 < n; a0 += kImHeadings) {                            // headings are independent: 64 per pass over W
        const int na = n - a0 < kImHeadings ? n - a0 : kImHeadings;
        HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)a0 * N, (size_t)na * N, hipMemcpyHostToDevice, c->stream));
        rc = infomax_score_device(c, c->d_sense, (long long)N, 1, 0, na, familiarity + a0);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    for (int a = 0; a < n; ++a) familiarity[a] = -familiarity[a];
    return DV_OK;
}

extern "C" int dv_infomax_sense_step(dv_ctx* c, double x, double y, const double* angles, int n, double* angle_fam, int32_t* best_heading) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_infomax_sense_step");
    if (rc) return rc;
    if (!angles || !angle_fam || !best_heading || n < 1) return fail(c, DV_ERR_INVALID, "dv_infomax_sense_step: NULL argument or n_headings < 1");
    rc = sensor_fits(c, "dv_infomax_sense_step", c->im_hh, c->im_ww);
    if (rc) return rc;
    if (!c->im_finite[0]) return infomax_not_finite(c, "dv_infomax_sense_step");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->im_N;
    rc = ensure_sense_buffer(c, (size_t)kImHeadings * N * 3);
    if (rc) return rc;
    double xs[kImHeadings], ys[kImHeadings];
    for (int a = 0; a < kImHeadings; ++a) { xs[a] = x; ys[a] = y; }
    for (int a0 = 0; a0 < n; a0 += kImHeadings) {
        const int na = n - a0 < kImHeadings ? n - a0 : kImHeadings;
        rc = enqueue_sense(c, xs, ys, angles + a0, na, c->d_sense);
        if (rc) return rc;
        rc = infomax_score_device(c, c->d_sense, 3ll * (long long)N, 3, c->im_channel, na, angle_fam + a0);
        if (rc) return rc;
        rc = check_sense_error(c);                                           // (synchronises)
        if (rc) return rc;
    }
    int best = 0;
    for (int a = 0; a < n; ++a) {
        angle_fam[a] = -angle_fam[a];
        if (angle_fam[a] > angle_fam[best]) best = a;                        // first maximum, as np.argmax
    }
    *best_heading = best;
    return DV_OK;
}

// ---- ensembles: every member's headings in one enqueue and one wait ----------------------------------------------------------
static constexpr long long kImSlabColsMax = 1 << 20;          // columns of one scoring launch (its grid's y extent: 16384 blocks)

// planes != nullptr: uploaded uint8[n_agents][A][h][w]; else the poses (x[i], y[i], angles[i][a]) are sensed.  The unfused pair (sense,
// then k_im_prep over the slab's patches in one launch) keeps x's bits by construction.  Columns go through X in slabs of at most
// kImStageBytes, back to back on the stream; the host waits once, for the one copy of the packed results.
static int infomax_batch(dv_ctx* c, const char* who, const uint8_t* planes, const double* x, const double* y, const double* angles, int n_agents,
                         int A, double* angle_fam, int32_t* best_heading, uint32_t* flags) {
    const long long C = (long long)n_agents * A;
    if (C > 0x7fffffffll - kImHeadings) return fail(c, DV_ERR_INVALID, "%s: %d agents x %d headings are too many columns", who, n_agents, A);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->im_N;
    const int M = c->im_M, tiles = (M + 15) / 16;
    const long long cpad = (C + kImHeadings - 1) / kImHeadings * kImHeadings;
    long long slab = (long long)(kImStageBytes / (N * sizeof(double))) / kImHeadings * kImHeadings;
    if (slab < kImHeadings) slab = kImHeadings;
    if (slab > kImSlabColsMax) slab = kImSlabColsMax;
    if (slab > cpad) slab = cpad;
    double* d_fam = nullptr; int* d_best = nullptr; unsigned* d_flags = nullptr;   // the packed results' parts on the device
    int rc = grow_buffer(c, c->im_bx, c->im_bx_cap, (size_t)slab * N * sizeof(double));
    if (!rc) rc = grow_buffer(c, c->im_bdpart, c->im_bdpart_cap, (size_t)tiles * (size_t)cpad * sizeof(double));
    if (!rc) rc = packed_device(c, c->im_res, C, n_agents, d_fam, d_best, d_flags);
    if (!rc && !planes) rc = grow_buffer(c, c->im_perr, c->im_perr_cap, (size_t)C * sizeof(int));
    if (!rc) rc = ensure_sense_buffer(c, (size_t)slab * N * (planes ? 1 : 3));
    if (rc) return rc;
    if (!planes) {
        rc = upload_member_poses(c, x, y, angles, n_agents, A);
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(c->im_perr, 0, (size_t)C * sizeof(int), c->stream));
    }
    for (long long c0 = 0; c0 < C; c0 += slab) {
        const long long nc = C - c0 < slab ? C - c0 : slab;
        if (planes) {
            HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)c0 * N, (size_t)nc * N, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_im_prep, dim3((unsigned)nc), dim3(256), 0, c->stream, c->d_sense, (long long)N, 1, 0, c->im_N, c->im_bx);
        } else {
            const long long total = nc * (long long)N;
            hipLaunchKernelGGL(k_sense_each, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->d_land, c->d_poses + c0, (int)nc,
                               c->sensor, c->d_lut, c->d_sense, c->im_perr + c0);
            HIP_TRY(c, hipGetLastError());
            hipLaunchKernelGGL(k_im_prep, dim3((unsigned)nc), dim3(256), 0, c->stream, c->d_sense, 3ll * (long long)N, 3, c->im_channel, c->im_N,
                               c->im_bx);
        }
        HIP_TRY(c, hipGetLastError());
        const dim3 grid((unsigned)tiles, (unsigned)((nc + kImHeadings - 1) / kImHeadings));
        if (N % 4 == 0)
            hipLaunchKernelGGL((k_im_score_cols<true>), grid, dim3(kImScoreWaves * 64), 0, c->stream, c->im_W, c->im_bx, M, c->im_N, (int)nc, cpad,
                               c->im_bdpart + c0);
        else
            hipLaunchKernelGGL((k_im_score_cols<false>), grid, dim3(kImScoreWaves * 64), 0, c->stream, c->im_W, c->im_bx, M, c->im_N, (int)nc, cpad,
                               c->im_bdpart + c0);
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_im_decide, dim3((unsigned)n_agents), dim3(256), 0, c->stream, c->im_bdpart, tiles, cpad, A, planes ? nullptr : c->im_perr,
                       d_fam, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    rc = packed_fetch(c, c->im_res, C, n_agents);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    packed_unpack(c->im_res, C, n_agents, angle_fam, best_heading, flags);
    return DV_OK;
}

extern "C" int dv_batch_infomax_step_u8(dv_ctx* c, const uint8_t* planes, int n_agents, int n_headings, double* angle_fam, int32_t* best_heading) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_batch_infomax_step_u8");
    if (rc) return rc;
    if (!planes || !angle_fam || !best_heading || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_batch_infomax_step_u8: NULL argument, n_agents < 1 or n_headings < 1");
    if (!c->im_finite[0]) return infomax_not_finite(c, "dv_batch_infomax_step_u8");
    return infomax_batch(c, "dv_batch_infomax_step_u8", planes, nullptr, nullptr, nullptr, n_agents, n_headings, angle_fam, best_heading, nullptr);
}

extern "C" int dv_batch_infomax_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                           double* angle_fam, int32_t* best_heading, uint32_t* flags) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_batch_infomax_sense_step");
    if (rc) return rc;
    if (!x || !y || !angles || !angle_fam || !best_heading || !flags || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_batch_infomax_sense_step: NULL argument, n_agents < 1 or n_headings < 1");
    rc = sensor_fits(c, "dv_batch_infomax_sense_step", c->im_hh, c->im_ww);
    if (rc) return rc;
    if (!c->im_finite[0]) return infomax_not_finite(c, "dv_batch_infomax_sense_step");
    return infomax_batch(c, "dv_batch_infomax_sense_step", nullptr, x, y, angles, n_agents, n_headings, angle_fam, best_heading, flags);
}

extern "C" int dv_infomax_read_weights(dv_ctx* c, double* out) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_infomax_read_weights");
    if (rc) return rc;
    if (!out) return fail(c, DV_ERR_INVALID, "dv_infomax_read_weights: out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->im_W, (size_t)c->im_M * (size_t)c->im_N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DV_OK;
}

extern "C" int dv_infomax_set_weights(dv_ctx* c, const double* weights) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need_bank0(c, "dv_infomax_set_weights");
    if (rc) return rc;
    if (!weights) return fail(c, DV_ERR_INVALID, "dv_infomax_set_weights: weights is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->im_W, weights, (size_t)c->im_M * (size_t)c->im_N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return infomax_check_finite(c);
}

extern "C" int dv_infomax_info(dv_ctx* c, int* n_hidden, int* n_pixels, int64_t* views_trained, int* finite, int64_t* bytes) {
    if (!c) return DV_ERR_INVALID;
    if (n_hidden) *n_hidden = c->im_M;
    if (n_pixels) *n_pixels = c->im_N;
    if (views_trained) *views_trained = c->im_views[0];
    if (finite) *finite = c->im_W && c->im_finite[0] ? 1 : 0;
    if (bytes) *bytes = (int64_t)c->im_M * c->im_N * (int64_t)sizeof(double);
    return DV_OK;
}

// ---- weight banks: n_banks models of one shape and one learning rate (include/dejavu.h: dv_ibank_*) -------------------------------------
static constexpr int kImMaxBanks = 65535;                     // (the bank is a grid dimension)

// Every bank's im_finite from the weights as they stand, in one launch (synchronises the stream).
static int ibank_check_finite(dv_ctx* c) {
    const long long n = (long long)c->im_M * c->im_N;
    const size_t B = (size_t)c->im_banks;
    HIP_TRY(c, hipMemsetAsync(c->im_flag, 0, B * sizeof(int), c->stream));
    const long long blocks = (n + 255) / 256;
    if (c->inet_nets) {                                       // ragged banks: each over its own network's weights
        const int rc = inet_finite(c);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_im_finite_banks, dim3((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)B), dim3(256), 0, c->stream, c->im_W, n, c->im_flag);
        HIP_TRY(c, hipGetLastError());
    }
    std::vector<int> bad(B, 0);
    HIP_TRY(c, hipMemcpyAsync(bad.data(), c->im_flag, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t b = 0; b < B; ++b) c->im_finite[b] = bad[b] == 0;
    return DV_OK;
}

// A banked call's table, checked entry by entry before anything of the call reaches the device: first every entry's range, then that
// no entry names a bank whose weights are not finite.
static int ibank_check(dv_ctx* c, const char* who, const char* what, const int32_t* bank_of, int64_t n) {
    const int rc = index_check(c, who, what, bank_of, n, c->im_banks, "n_banks");
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (!c->im_finite[(size_t)bank_of[i]])
            return fail(c, DV_ERR_STATE, "%s: %s[%lld] names bank %d, whose weights are not finite (learning_rate %g is too large for its views: the rule diverged)",
                        who, what, (long long)i, (int)bank_of[i], ibank_eta(c, bank_of[i]));
    return DV_OK;
}

// After a banked training call: the first bank the call trained whose weights are no longer finite.
static int ibank_report(dv_ctx* c, const char* who, const int32_t* bank_of, int64_t n) {
    std::vector<char> named((size_t)c->im_banks, 0);
    for (int64_t v = 0; v < n; ++v) named[(size_t)bank_of[v]] = 1;
    for (int b = 0; b < c->im_banks; ++b)
        if (named[(size_t)b] && !c->im_finite[(size_t)b])
            return fail(c, DV_ERR_STATE, "%s: the weights of bank %d are not finite (learning_rate %g is too large for its views: the rule diverged)", who, b,
                        ibank_eta(c, b));
    return DV_OK;
}

// h, u and upart of every bank: made at the first banked training call after dv_infomax_begin / dv_ibank_set (dv_inet_set has made
// its own, ragged ones, and im_kh[0] holds them).
static int ibank_buffers(dv_ctx* c) {
    if (c->im_kh[0]) return DV_OK;
    const size_t B = (size_t)c->im_banks, M = (size_t)c->im_M, N = (size_t)c->im_N, n_rb = (M + kImRowsPerBlock - 1) / kImRowsPerBlock;
    hipError_t e = hipMalloc((void**)&c->im_kh[0], B * M * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_kh[1], B * M * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_ku, B * N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&c->im_kupart, B * n_rb * N * sizeof(double));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
        F(c->im_kh[0]); F(c->im_kh[1]); F(c->im_ku); F(c->im_kupart);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "Infomax banks: the training buffers of %zu banks: %s", B, hipGetErrorString(e));
    }
    return DV_OK;
}

// Enqueue the banks' training chains over n views resident on the device (layout as k_im_prep's src), view v into bank bank_of[v]: per
// slab of x vectors one k_im_prep over all its views, one k_im_gemv_banks for every chain's first h, then step s = the s-th view of every
// bank that has one, in three launches.
static int ibank_train_device(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, int offset, int64_t n, const int32_t* bank_of) {
    if (n < 1) return DV_OK;
    const int M = c->im_M, N = c->im_N, B = c->im_banks;
    int rc = infomax_stage_x(c);
    if (!rc) rc = ibank_buffers(c);
    if (rc) return rc;
    const int64_t cap = (int64_t)c->im_xs_cap, n_slabs = (n + cap - 1) / cap;
    const size_t idx0 = (size_t)n_slabs * 2 * (size_t)B;     // [slab][2][B] chain lengths and list starts, then the lists: n places in xs
    std::vector<int> t(idx0 + (size_t)n, 0), cur((size_t)B);
    for (int64_t k = 0; k < n_slabs; ++k) {
        int* len = t.data() + (size_t)k * 2 * (size_t)B;
        int* start = len + B;
        const int64_t b0 = k * cap, nb = n - b0 < cap ? n - b0 : cap;
        for (int64_t v = 0; v < nb; ++v) len[bank_of[b0 + v]] += 1;
        int run = (int)b0;
        for (int b = 0; b < B; ++b) { start[b] = cur[(size_t)b] = run; run += len[b]; }
        for (int64_t v = 0; v < nb; ++v) t[idx0 + (size_t)cur[(size_t)bank_of[b0 + v]]++] = (int)v;
    }
    if (c->inet_nets) t.insert(t.end(), bank_of, bank_of + n);   // then the views' banks: k_inet_prep reads a view at its bank's channel
    rc = table_upload(c, c->im_ktab, t.data(), t.size() * sizeof(int));
    if (rc) return rc;
    const int* d_idx = c->im_ktab.device<int>() + idx0;
    const double rate = c->im_eta / (double)N;
    const unsigned row_blocks = (unsigned)((M + 3) / 4), col_blocks = (unsigned)((N + 255) / 256);
    const int n_rb = (M + kImRowsPerBlock - 1) / kImRowsPerBlock;
    for (int64_t k = 0; k < n_slabs; ++k) {
        const int64_t b0 = k * cap, nb = n - b0 < cap ? n - b0 : cap;
        const int* len = c->im_ktab.record<int>() + (size_t)k * 2 * (size_t)B;
        const int* d_tab = c->im_ktab.device<int>() + (size_t)k * 2 * (size_t)B;
        int steps = 0;
        for (int b = 0; b < B; ++b) steps = len[b] > steps ? len[b] : steps;
        if (c->inet_nets) {                                   // (a strided source is the sensed views, read at the bank's own channel instead of `offset`)
            rc = inet_train_slab(c, d_src + (size_t)b0 * (size_t)view_stride, view_stride, px_stride, nb, d_tab, d_idx, d_idx + (size_t)n + (size_t)b0, steps);
            if (rc) return rc;
            continue;
        }
        hipLaunchKernelGGL(k_im_prep, dim3((unsigned)nb), dim3(256), 0, c->stream, d_src + (size_t)b0 * (size_t)view_stride, view_stride, px_stride,
                           offset, N, c->im_xs);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(k_im_gemv_banks, dim3(row_blocks, (unsigned)B), dim3(256), 0, c->stream, c->im_W, c->im_xs, M, N, c->im_kh[0], d_tab, d_idx);
        HIP_TRY(c, hipGetLastError());
        for (int s = 0; s < steps; ++s) {
            double* h = c->im_kh[s & 1];
            hipLaunchKernelGGL(k_im_upart_banks, dim3(col_blocks, (unsigned)n_rb, (unsigned)B), dim3(256), 0, c->stream, c->im_W, h, M, N, c->im_kupart,
                               d_tab, s);
            hipLaunchKernelGGL(k_im_ureduce_banks, dim3(col_blocks, (unsigned)B), dim3(256), 0, c->stream, c->im_kupart, n_rb, N, c->im_ku, d_tab, s);
            hipLaunchKernelGGL(k_im_update_banks, dim3(row_blocks, (unsigned)B), dim3(256), 0, c->stream, c->im_W, h, c->im_ku, M, N, rate, c->im_xs,
                               c->im_kh[(s & 1) ^ 1], d_tab, d_idx, s);
            HIP_TRY(c, hipGetLastError());
        }
    }
    for (int64_t v = 0; v < n; ++v) c->im_views[(size_t)bank_of[v]] += 1;
    return DV_OK;
}

// An ensemble's step under banks: member i's columns multiply the weights of bank bank_of[i].  The host sorts the members by bank
// (stably), hands the device their patches or poses in that order and a table of column blocks that never mix banks; k_im_decide_banks
// maps the columns back, so the results come in the caller's order.  One enqueue, one wait, as infomax_batch.
// land_of != nullptr (poses only): member i senses landscape land_of[i] of the set (dejavu_lands.inl); the table rides the members'
// permutation, so the device's entry p is the landscape of the member at place p, and k_sense_lands indexes it by the sorted column.
static int ibank_batch(dv_ctx* c, const char* who, const uint8_t* planes, const double* x, const double* y, const double* angles, int n_agents, int A,
                       const int32_t* bank_of, const int32_t* land_of, double* angle_fam, int32_t* best_heading, uint32_t* flags) {
    int rc = ibank_check(c, who, "bank_of_member", bank_of, n_agents);
    if (rc) return rc;
    if (land_of) { rc = lands_check(c, who, "land_of_member", land_of, n_agents); if (rc) return rc; }
    else if (!planes) { rc = noise_need_lands(c, who); if (rc) return rc; }
    const long long C = (long long)n_agents * A;
    const int B = c->im_banks;
    if (C + (long long)kImHeadings * B > 0x7fffffffll - kImHeadings)
        return fail(c, DV_ERR_INVALID, "%s: %d agents x %d headings over %d banks are too many columns", who, n_agents, A, B);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->im_N;
    const int M = c->im_M, tiles = ((c->inet_nets ? c->inet_max_M : M) + 15) / 16;   // (a table's grids and dpart: its largest n_hidden)
    // members in bank order: place[i] of member i, order[p] the member at place p; first[b] the first place of bank b
    std::vector<int> first((size_t)B + 1, 0), place((size_t)n_agents), order((size_t)n_agents), dbase((size_t)B);
    for (int i = 0; i < n_agents; ++i) first[(size_t)bank_of[i] + 1] += 1;
    for (int b = 0; b < B; ++b) first[(size_t)b + 1] += first[(size_t)b];
    {
        std::vector<int> cur(first.begin(), first.end() - 1);
        for (int i = 0; i < n_agents; ++i) { place[(size_t)i] = cur[(size_t)bank_of[i]]++; order[(size_t)place[(size_t)i]] = i; }
    }
    // the table: column blocks {bank, first column of X, columns, first column of dpart}, then per member of the caller's order
    // {first column in dpart, first column in X}
    long long cpad = 0;
    std::vector<int> t;
    for (int b = 0; b < B; ++b) {
        const long long cols = (long long)(first[(size_t)b + 1] - first[(size_t)b]) * A, x0 = (long long)first[(size_t)b] * A;
        dbase[(size_t)b] = (int)cpad;
        for (long long o = 0; o < cols; o += kImHeadings) {
            const int bk[4] = {b, (int)(x0 + o), (int)(cols - o < kImHeadings ? cols - o : kImHeadings), (int)(cpad + o)};
            t.insert(t.end(), bk, bk + 4);
        }
        cpad += (cols + kImHeadings - 1) / kImHeadings * kImHeadings;
    }
    const size_t n_blocks = t.size() / 4;
    for (int i = 0; i < n_agents; ++i) {
        const int b = bank_of[i];
        t.push_back(dbase[(size_t)b] + (place[(size_t)i] - first[(size_t)b]) * A);
        t.push_back(place[(size_t)i] * A);
    }
    if (c->inet_nets) {                                       // then the members' banks, in the caller's order (k_inet_decide) and in bank order (k_inet_prep)
        t.insert(t.end(), bank_of, bank_of + n_agents);
        for (int p = 0; p < n_agents; ++p) t.push_back(bank_of[(size_t)order[(size_t)p]]);
    }
    long long slab = (long long)(kImStageBytes / (N * sizeof(double))) / kImHeadings * kImHeadings;
    if (slab < kImHeadings) slab = kImHeadings;
    if (slab > kImSlabColsMax) slab = kImSlabColsMax;
    if (slab > cpad) slab = cpad;
    double* d_fam = nullptr; int* d_best = nullptr; unsigned* d_flags = nullptr;
    rc = grow_buffer(c, c->im_bx, c->im_bx_cap, (size_t)slab * N * sizeof(double));
    if (!rc) rc = grow_buffer(c, c->im_bdpart, c->im_bdpart_cap, (size_t)tiles * (size_t)cpad * sizeof(double));
    if (!rc) rc = packed_device(c, c->im_res, C, n_agents, d_fam, d_best, d_flags);
    if (!rc && !planes) rc = grow_buffer(c, c->im_perr, c->im_perr_cap, (size_t)C * sizeof(int));
    if (!rc) rc = ensure_sense_buffer(c, (size_t)slab * N * (planes ? 1 : 3));
    if (!rc) rc = table_upload(c, c->im_ktab, t.data(), t.size() * sizeof(int));
    if (!rc && land_of) {
        std::vector<int32_t> sorted((size_t)n_agents);
        for (int p = 0; p < n_agents; ++p) sorted[(size_t)p] = land_of[(size_t)order[(size_t)p]];
        rc = lands_upload(c, sorted.data(), n_agents, order.data());   // (live noise rows ride the same permutation)
    }
    if (rc) return rc;
    const ImBlock* blocks = c->im_ktab.record<ImBlock>();
    const ImBlock* d_blocks = c->im_ktab.device<ImBlock>();
    const int* d_mem = c->im_ktab.device<int>() + 4 * n_blocks;   // the members' pairs; under a network table their banks follow
    const int* d_bank_caller = c->inet_nets ? d_mem + 2 * (size_t)n_agents : nullptr, *d_bank_sorted = c->inet_nets ? d_bank_caller + n_agents : nullptr;
    if (planes) {
        c->im_kplanes.resize((size_t)C * N);
        for (int p = 0; p < n_agents; ++p)
            std::memcpy(c->im_kplanes.data() + (size_t)p * A * N, planes + (size_t)order[(size_t)p] * A * N, (size_t)A * N);
    } else {
        c->im_kpose.resize(2 * (size_t)n_agents + (size_t)C);
        double* xp = c->im_kpose.data(), *yp = xp + n_agents, *ap = yp + n_agents;
        for (int p = 0; p < n_agents; ++p) {
            const size_t i = (size_t)order[(size_t)p];
            xp[p] = x[i];
            yp[p] = y[i];
            std::memcpy(ap + (size_t)p * A, angles + i * A, (size_t)A * sizeof(double));
        }
        rc = upload_member_poses(c, xp, yp, ap, n_agents, A);
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(c->im_perr, 0, (size_t)C * sizeof(int), c->stream));
    }
    for (size_t k0 = 0; k0 < n_blocks;) {                    // a slab: consecutive blocks, so consecutive columns of X
        const long long c0 = blocks[k0].x0;
        long long nc = 0;
        size_t nk = 0;
        while (k0 + nk < n_blocks && nk < (size_t)(kImSlabColsMax / kImHeadings) && nc + blocks[k0 + nk].nc <= slab) nc += blocks[k0 + nk++].nc;
        if (planes) {
            HIP_TRY(c, hipMemcpyAsync(c->d_sense, c->im_kplanes.data() + (size_t)c0 * N, (size_t)nc * N, hipMemcpyHostToDevice, c->stream));
            if (c->inet_nets) { rc = inet_prep(c, c->d_sense, (long long)N, 1, 0, nc, c->im_bx, d_bank_sorted, c0, A); if (rc) return rc; }
            else hipLaunchKernelGGL(k_im_prep, dim3((unsigned)nc), dim3(256), 0, c->stream, c->d_sense, (long long)N, 1, 0, c->im_N, c->im_bx);
        } else {
            const long long total = nc * (long long)N;
            if (land_of) {
                rc = lands_launch_sense(c, c0, c0, A, nc, c->d_sense, c->im_perr + c0);
                if (rc) return rc;
            } else {
                hipLaunchKernelGGL(k_sense_each, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->d_land, c->d_poses + c0, (int)nc,
                                   c->sensor, c->d_lut, c->d_sense, c->im_perr + c0);
                HIP_TRY(c, hipGetLastError());
            }
            if (c->inet_nets) { rc = inet_prep(c, c->d_sense, 3ll * (long long)N, 3, 1, nc, c->im_bx, d_bank_sorted, c0, A); if (rc) return rc; }
            else hipLaunchKernelGGL(k_im_prep, dim3((unsigned)nc), dim3(256), 0, c->stream, c->d_sense, 3ll * (long long)N, 3, c->im_channel, c->im_N,
                                    c->im_bx);
        }
        HIP_TRY(c, hipGetLastError());
        const dim3 grid((unsigned)tiles, (unsigned)nk);
        if (c->inet_nets) { rc = inet_score(c, d_blocks + k0, nk, c0, cpad); if (rc) return rc; }
        else if (N % 4 == 0)
            hipLaunchKernelGGL((k_im_score_cols_banks<true>), grid, dim3(kImScoreWaves * 64), 0, c->stream, c->im_W, c->im_bx, M, c->im_N, d_blocks + k0,
                               (int)c0, cpad, c->im_bdpart);
        else
            hipLaunchKernelGGL((k_im_score_cols_banks<false>), grid, dim3(kImScoreWaves * 64), 0, c->stream, c->im_W, c->im_bx, M, c->im_N, d_blocks + k0,
                               (int)c0, cpad, c->im_bdpart);
        HIP_TRY(c, hipGetLastError());
        k0 += nk;
    }
    if (c->inet_nets) { rc = inet_decide(c, n_agents, cpad, A, planes ? nullptr : c->im_perr, d_mem, d_bank_caller, d_fam, d_best, d_flags); if (rc) return rc; }
    else hipLaunchKernelGGL(k_im_decide_banks, dim3((unsigned)n_agents), dim3(256), 0, c->stream, c->im_bdpart, tiles, cpad, A,
                            planes ? nullptr : c->im_perr, d_mem, d_fam, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    rc = packed_fetch(c, c->im_res, C, n_agents);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    packed_unpack(c->im_res, C, n_agents, angle_fam, best_heading, flags);
    return DV_OK;
}

extern "C" int dv_ibank_set(dv_ctx* c, int n_banks, const double* w0) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need(c, "dv_ibank_set");
    if (rc) return rc;
    if (n_banks < 1 || n_banks > kImMaxBanks) return fail(c, DV_ERR_INVALID, "dv_ibank_set: n_banks %d outside [1, %d]", n_banks, kImMaxBanks);
    if (!w0) return fail(c, DV_ERR_INVALID, "dv_ibank_set: the initial weights are NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t mn = (size_t)c->im_M * (size_t)c->im_N, wbytes = mn * sizeof(double);
    double* W = nullptr;
    int* flag = nullptr;
    hipError_t e = hipMalloc((void**)&W, (size_t)n_banks * wbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&flag, (size_t)n_banks * sizeof(int));
    if (e == hipSuccess) e = hipMemcpyAsync(W, w0, wbytes, hipMemcpyHostToDevice, c->stream);
    for (int b = 1; b < n_banks && e == hipSuccess; ++b) e = hipMemcpyAsync(W + (size_t)b * mn, W, wbytes, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // `w0` is borrowed for this call only; nothing reads the old weights any more
    if (e != hipSuccess) {                                              // the model stays as it was
        (void)hipGetLastError();
        if (W) (void)hipFree(W);
        if (flag) (void)hipFree(flag);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_ibank_set: %d banks of %d x %d weights: %s", n_banks, c->im_M, c->im_N,
                    hipGetErrorString(e));
    }
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->im_W); F(c->im_flag); F(c->im_kh[0]); F(c->im_kh[1]); F(c->im_ku); F(c->im_kupart);   // (the banked buffers are per bank: made again at need)
    c->im_W = W;
    c->im_flag = flag;
    c->im_banks = n_banks;
    c->im_views.assign((size_t)n_banks, 0);
    c->im_finite.assign((size_t)n_banks, 1);
    inet_drop(c);                                             // the banks are the begin's network's again
    return ibank_check_finite(c);
}

extern "C" int dv_ibank_train_u8(dv_ctx* c, const uint8_t* planes, int64_t n, const int32_t* bank_of_view) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need(c, "dv_ibank_train_u8");
    if (rc) return rc;
    if (!planes || n < 0 || n > 0x7fffffff) return fail(c, DV_ERR_INVALID, "dv_ibank_train_u8: planes is NULL or n outside [0, 2^31)");
    rc = ibank_check(c, "dv_ibank_train_u8", "bank_of_view", bank_of_view, n);
    if (rc) return rc;
    if (n == 0) return DV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->im_N;
    size_t slab = kImStageBytes / N;
    if (slab < 1) slab = 1;
    if ((int64_t)slab > n) slab = (size_t)n;
    rc = ensure_sense_buffer(c, slab * N);
    if (rc) return rc;
    for (int64_t v0 = 0; v0 < n; v0 += (int64_t)slab) {
        const int64_t ns = n - v0 < (int64_t)slab ? n - v0 : (int64_t)slab;
        HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)v0 * N, (size_t)ns * N, hipMemcpyHostToDevice, c->stream));
        rc = ibank_train_device(c, c->d_sense, (long long)N, 1, 0, ns, bank_of_view + v0);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // the slab is reused, `planes` is borrowed
    }
    rc = ibank_check_finite(c);
    if (rc) return rc;
    return ibank_report(c, "dv_ibank_train_u8", bank_of_view, n);
}

// land_of == nullptr: the poses are on the context's one landscape (k_sense); else pose v is on landscape land_of[v] of the set.
static int ibank_train_from_poses(dv_ctx* c, const char* who, const double* x, const double* y, const double* angle, int64_t n,
                                  const int32_t* bank_of_view, const int32_t* land_of, uint8_t* out_views) {
    int rc = infomax_need(c, who);
    if (rc) return rc;
    if (!x || !y || !angle || n < 1 || n > 0x7fffffff) return fail(c, DV_ERR_INVALID, "%s: bad arguments", who);
    rc = sensor_fits(c, who, c->im_hh, c->im_ww);
    if (rc) return rc;
    rc = ibank_check(c, who, "bank_of_view", bank_of_view, n);
    if (rc) return rc;
    if (land_of) { rc = lands_check(c, who, "land_of_view", land_of, n); if (rc) return rc; }
    else { rc = noise_need_lands(c, who); if (rc) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * (size_t)c->im_N * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (!rc && land_of) rc = lands_upload(c, land_of, n);
    if (rc) return rc;
    rc = land_of ? lands_enqueue_sense(c, x, y, angle, n) : enqueue_sense(c, x, y, angle, n, c->d_sense);
    if (rc) return rc;
    if (out_views) HIP_TRY(c, hipMemcpyAsync(out_views, c->d_sense, bytes, hipMemcpyDeviceToHost, c->stream));
    rc = land_of ? lands_check_sense_error(c, who, n) : check_sense_error(c);   // DV_ERR_INDEX: no bank has been trained on anything
    if (rc) return rc;
    rc = ibank_train_device(c, c->d_sense, 3ll * c->im_N, 3, c->im_channel, n, bank_of_view);
    if (rc) return rc;
    rc = ibank_check_finite(c);
    if (rc) return rc;
    return ibank_report(c, who, bank_of_view, n);
}

extern "C" int dv_ibank_train_from_poses(dv_ctx* c, const double* x, const double* y, const double* angle, int64_t n, const int32_t* bank_of_view,
                                         uint8_t* out_views) {
    if (!c) return DV_ERR_INVALID;
    return ibank_train_from_poses(c, "dv_ibank_train_from_poses", x, y, angle, n, bank_of_view, nullptr, out_views);
}

extern "C" int dv_lands_ibank_train_from_poses(dv_ctx* c, const double* x, const double* y, const double* angle, int64_t n,
                                               const int32_t* bank_of_view, const int32_t* land_of_view, uint8_t* out_views) {
    if (!c) return DV_ERR_INVALID;
    if (!land_of_view) return fail(c, DV_ERR_INVALID, "dv_lands_ibank_train_from_poses: land_of_view is NULL");
    return ibank_train_from_poses(c, "dv_lands_ibank_train_from_poses", x, y, angle, n, bank_of_view, land_of_view, out_views);
}

extern "C" int dv_ibank_step_u8(dv_ctx* c, const uint8_t* planes, int n_agents, int n_headings, const int32_t* bank_of_member, double* angle_fam,
                                int32_t* best_heading) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need(c, "dv_ibank_step_u8");
    if (rc) return rc;
    if (!planes || !bank_of_member || !angle_fam || !best_heading || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_ibank_step_u8: NULL argument, n_agents < 1 or n_headings < 1");
    return ibank_batch(c, "dv_ibank_step_u8", planes, nullptr, nullptr, nullptr, n_agents, n_headings, bank_of_member, nullptr, angle_fam, best_heading, nullptr);
}

extern "C" int dv_ibank_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                   const int32_t* bank_of_member, double* angle_fam, int32_t* best_heading, uint32_t* flags) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need(c, "dv_ibank_sense_step");
    if (rc) return rc;
    if (!x || !y || !angles || !bank_of_member || !angle_fam || !best_heading || !flags || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_ibank_sense_step: NULL argument, n_agents < 1 or n_headings < 1");
    rc = sensor_fits(c, "dv_ibank_sense_step", c->im_hh, c->im_ww);
    if (rc) return rc;
    return ibank_batch(c, "dv_ibank_sense_step", nullptr, x, y, angles, n_agents, n_headings, bank_of_member, nullptr, angle_fam, best_heading, flags);
}

extern "C" int dv_lands_ibank_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                         const int32_t* bank_of_member, const int32_t* land_of_member, double* angle_fam, int32_t* best_heading,
                                         uint32_t* flags) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need(c, "dv_lands_ibank_sense_step");
    if (rc) return rc;
    if (!x || !y || !angles || !bank_of_member || !land_of_member || !angle_fam || !best_heading || !flags || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_lands_ibank_sense_step: NULL argument, n_agents < 1 or n_headings < 1");
    rc = sensor_fits(c, "dv_lands_ibank_sense_step", c->im_hh, c->im_ww);
    if (rc) return rc;
    return ibank_batch(c, "dv_lands_ibank_sense_step", nullptr, x, y, angles, n_agents, n_headings, bank_of_member, land_of_member, angle_fam,
                       best_heading, flags);
}

static int ibank_one(dv_ctx* c, const char* who, int bank) {
    int rc = infomax_need(c, who);
    if (rc) return rc;
    if (bank < 0 || bank >= c->im_banks) return fail(c, DV_ERR_INVALID, "%s: bank %d outside [0, n_banks = %d)", who, bank, c->im_banks);
    return DV_OK;
}

extern "C" int dv_ibank_read_weights(dv_ctx* c, int bank, double* out) {
    if (!c) return DV_ERR_INVALID;
    int rc = ibank_one(c, "dv_ibank_read_weights", bank);
    if (rc) return rc;
    if (!out) return fail(c, DV_ERR_INVALID, "dv_ibank_read_weights: out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    size_t off, mn;
    ibank_span(c, bank, off, mn);
    HIP_TRY(c, hipMemcpyAsync(out, c->im_W + off, mn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DV_OK;
}

extern "C" int dv_ibank_set_weights(dv_ctx* c, int bank, const double* weights) {
    if (!c) return DV_ERR_INVALID;
    int rc = ibank_one(c, "dv_ibank_set_weights", bank);
    if (rc) return rc;
    if (!weights) return fail(c, DV_ERR_INVALID, "dv_ibank_set_weights: weights is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    size_t off, mn;
    ibank_span(c, bank, off, mn);
    HIP_TRY(c, hipMemcpyAsync(c->im_W + off, weights, mn * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return infomax_check_finite(c, bank);                     // (synchronises: `weights` is borrowed for this call only)
}

extern "C" int dv_ibank_info(dv_ctx* c, int* n_banks, int64_t* views_trained, int32_t* finite) {
    if (!c) return DV_ERR_INVALID;
    if (n_banks) *n_banks = c->im_banks;
    for (size_t b = 0; b < (size_t)c->im_banks; ++b) {
        if (views_trained) views_trained[b] = c->im_views[b];
        if (finite) finite[b] = c->im_W && c->im_finite[b] ? 1 : 0;
    }
    return DV_OK;
}
