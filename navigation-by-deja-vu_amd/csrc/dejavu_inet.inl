// Network tables of the Infomax model (include/dejavu.h: dv_inet_*): a weight bank with hidden units, learning rate, initial weights and
// compared channel of its own.  A network is (channel, M = n_hidden, learning_rate, W0 double[M][N]); the table gives the engine P
// networks and B banks, network_of_bank[b] naming bank b's.  The views' h x w, so N, stay the ones dv_infomax_begin fixed.
//
// The device keeps one descriptor per BANK (InetBank, 48 bytes: its own W, h, upart, rate, M, row blocks, channel), read at the
// workgroup's bank -- a grid dimension in training, the column block's bank in a step -- so it is the same for every lane of the
// workgroup and a scalar load.  u is not in it: it has N doubles for every bank, so bank b's is u + b N; nor is the second h, which lies
// h_stride doubles behind the first for every bank.  Everything after the descriptor is the device function of the banked twin
// (dejavu_infomax.inl) on the descriptor's values, so there stays one statement of every sum and its order:
//
//   k_inet_prep      k_im_prep's body (im_prep_view) with the compared channel of the view's bank: banks of different channels share a
//                    slab of sensed views.  by_channel: the source is the sensed uint8[n][h][w][3]; else the bytes are the plane already.
//   k_inet_gemv, k_inet_upart, k_inet_ureduce, k_inet_update   k_im_*_banks on the bank's own W, M, row blocks and rate
//   k_inet_finite    k_im_finite_banks over the bank's own M N
//   k_inet_score_cols<VEC>   k_im_score_cols_banks on the block's bank; k_inet_decide   k_im_decide_banks over the bank's own row tiles
//
// Grids are sized for the largest M of the table.  A workgroup whose rows (gemv, update), row block (upart) or row tile (score) lie
// past its own bank's M leaves as a whole, after the descriptor's scalar loads and before any other load, store or barrier; ureduce sums
// the bank's own row blocks and decide the bank's own row tiles.  So nothing reads a partial sum that an engine of that M alone would
// not have, and bank b ends with that engine's bits.
//
// Weights are ragged: bank b's double[M_b][N] begins at N * (the sum of its predecessors' M), no padding; h and upart likewise.
namespace dv {

// Pointers read from memory are flat to the compiler; typed as what they are, global memory, the loads and stores through them are
// the global ones a kernel argument gets (as dejavu_mbpop.inl's descriptor).
#define DV_INET_GLOBAL __attribute__((address_space(1)))

struct InetBank {
    double DV_INET_GLOBAL* W;                  // [M][N]: the bank's own weights
    double DV_INET_GLOBAL* h;                  // [M], and [M] again h_stride doubles on: h of the current view and of the next
    double DV_INET_GLOBAL* upart;              // [n_row_blocks][N]
    double rate;                               // learning_rate / N, computed on the host as the single model's
    int M, n_row_blocks, channel, pad;
};
static_assert(sizeof(InetBank) == 48, "InetBank is 48 bytes");

// k_im_prep's body for the one view whose compared plane is p[j * px_stride], j < N: the same 256 strided partial sums, the same tree
// in LDS, / 255.0, minus the mean.  red: 256 doubles of LDS.
__device__ __forceinline__ void im_prep_view(const unsigned char* __restrict__ p, int px_stride, int N, double* __restrict__ xo, double* red) {
    const int tid = (int)threadIdx.x;
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

// View blockIdx.x of the launch belongs to bank bank_of[(col0 + blockIdx.x) / per]: per = 1 and the call's views in training, per = A
// and the members in bank order in a step.
__global__ __launch_bounds__(256) void k_inet_prep(const unsigned char* __restrict__ src, long long view_stride, int px_stride, int by_channel, int N,
                                                   double* __restrict__ x, const InetBank* __restrict__ desc, const int* __restrict__ bank_of,
                                                   unsigned col0, unsigned per) {
    __shared__ double red[256];
    const int offset = by_channel ? desc[bank_of[(col0 + blockIdx.x) / per]].channel : 0;
    im_prep_view(src + (size_t)blockIdx.x * (size_t)view_stride + offset, px_stride, N, x + (size_t)blockIdx.x * (size_t)N, red);
}

// tab, idx: the slab's chains, as k_im_gemv_banks takes them.  A slab's first h is the first of the two; cur (below): which of the two
// step s reads (the other is written).
__global__ __launch_bounds__(256) void k_inet_gemv(const double* __restrict__ xs, int N, const InetBank* __restrict__ desc, const int* __restrict__ tab,
                                                   const int* __restrict__ idx) {
    const int b = (int)blockIdx.y;
    if (tab[b] < 1) return;
    const InetBank k = desc[b];
    if ((int)blockIdx.x * 4 >= k.M) return;
    im_gemv_rows((const double*)k.W, xs + (size_t)idx[tab[gridDim.y + b]] * (size_t)N, k.M, N, (double*)k.h);
}

__global__ __launch_bounds__(256) void k_inet_upart(int N, int cur, long long h_stride, const InetBank* __restrict__ desc, const int* __restrict__ tab,
                                                    int s) {
    const int b = (int)blockIdx.z;
    if (s >= tab[b]) return;
    const InetBank k = desc[b];
    if ((int)blockIdx.y >= k.n_row_blocks) return;
    im_upart_cols((const double*)k.W, (const double*)k.h + (size_t)cur * (size_t)h_stride, k.M, N, (double*)k.upart);
}

__global__ __launch_bounds__(256) void k_inet_ureduce(int N, double* __restrict__ u, const InetBank* __restrict__ desc, const int* __restrict__ tab, int s) {
    const int b = (int)blockIdx.y;
    if (s >= tab[b]) return;
    const InetBank k = desc[b];
    im_ureduce_cols((const double*)k.upart, k.n_row_blocks, N, u + (size_t)b * (size_t)N);
}

__global__ __launch_bounds__(256) void k_inet_update(int N, int cur, long long h_stride, const double* __restrict__ u, const double* __restrict__ xs,
                                                     const InetBank* __restrict__ desc, const int* __restrict__ tab, const int* __restrict__ idx, int s) {
    const int b = (int)blockIdx.y, len = tab[b];
    if (s >= len) return;
    const InetBank k = desc[b];
    if ((int)blockIdx.x * 4 >= k.M) return;
    const double* x_next = s + 1 < len ? xs + (size_t)idx[tab[gridDim.y + b] + s + 1] * (size_t)N : nullptr;
    double* h = (double*)k.h;
    im_update_rows((double*)k.W, h + (size_t)cur * (size_t)h_stride, u + (size_t)b * (size_t)N, k.M, N, k.rate, x_next,
                   h + (size_t)(cur ^ 1) * (size_t)h_stride);
}

// flag: a word per bank (blockIdx.y)
__global__ __launch_bounds__(256) void k_inet_finite(const InetBank* __restrict__ desc, int N, int* __restrict__ flag) {
    const InetBank k = desc[blockIdx.y];
    if (im_any_not_finite((const double*)k.W, (long long)k.M * N)) flag[blockIdx.y] = 1;
}

template <bool VEC>
__global__ __launch_bounds__(kImScoreWaves * 64) void k_inet_score_cols(const double* __restrict__ X, int N, const InetBank* __restrict__ desc,
                                                                        const ImBlock* __restrict__ blocks, int x_first, long long cpad,
                                                                        double* __restrict__ dpart) {
    __shared__ double sred[16 * kImHeadings];
    const ImBlock bk = blocks[blockIdx.y];                               // (uniform over the workgroup)
    const InetBank k = desc[bk.bank];
    if ((int)blockIdx.x * 16 >= k.M) return;                             // a row tile the bank does not have: nobody reads its partials
    const double* Wb = (const double*)k.W;
    const double* Xb = X + (size_t)(bk.x0 - x_first) * (size_t)N;
    double* dout = dpart + (size_t)blockIdx.x * (size_t)cpad + bk.d0;
    if (bk.nc <= 16) im_score_tile<1, VEC>(Wb, Xb, k.M, N, bk.nc, (int)blockIdx.x, sred, dout);
    else if (bk.nc <= 32) im_score_tile<2, VEC>(Wb, Xb, k.M, N, bk.nc, (int)blockIdx.x, sred, dout);
    else im_score_tile<4, VEC>(Wb, Xb, k.M, N, bk.nc, (int)blockIdx.x, sred, dout);
}

// mem: as k_im_decide_banks takes it; bank_of: the bank of member blockIdx.x of the CALLER's order, whose own row tiles are summed.
__global__ __launch_bounds__(256) void k_inet_decide(const double* __restrict__ dpart, long long cpad, int A, const int* __restrict__ perr,
                                                     const int* __restrict__ mem, const int* __restrict__ bank_of, const InetBank* __restrict__ desc,
                                                     double* __restrict__ fam, int* __restrict__ best, unsigned* __restrict__ flags) {
    const int n_tiles = (desc[bank_of[blockIdx.x]].M + 15) / 16;
    im_decide_member(dpart, n_tiles, cpad, A, perr, (size_t)mem[2 * blockIdx.x], (size_t)mem[2 * blockIdx.x + 1],
                     fam + (size_t)blockIdx.x * (size_t)A, best + blockIdx.x, flags + blockIdx.x);
}

}  // namespace dv

// Forget the table (not the weights and buffers: the caller replaces or frees those).
static void inet_drop(dv_ctx* c) {
    table_free(c->inet_desc);
    c->inet_nets = 0;
    c->inet_max_M = 0;
    c->inet_h_stride = 0;
    c->inet_bytes = 0;
    c->inet_M.clear(); c->inet_channel.clear(); c->inet_eta.clear(); c->inet_of_bank.clear(); c->inet_row0.clear();
}

static int inet_prep(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, int by_channel, long long n, double* x,
                     const int* d_bank_of, long long col0, int per) {
    hipLaunchKernelGGL(k_inet_prep, dim3((unsigned)n), dim3(256), 0, c->stream, d_src, view_stride, px_stride, by_channel, c->im_N, x,
                       c->inet_desc.device<dv::InetBank>(), d_bank_of, (unsigned)col0, (unsigned)per);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// One slab of ibank_train_device under a live table: nb views at d_src, whose banks are d_bank_of[0 .. nb); d_tab, d_idx: the slab's
// chains; steps: the longest chain.  The launches of the path without a table, one for one.
static int inet_train_slab(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, long long nb, const int* d_tab, const int* d_idx,
                           const int* d_bank_of, int steps) {
    const int N = c->im_N, B = c->im_banks, M = c->inet_max_M;
    const dv::InetBank* desc = c->inet_desc.device<dv::InetBank>();
    const long long hs = (long long)c->inet_h_stride;
    const unsigned row_blocks = (unsigned)((M + 3) / 4), col_blocks = (unsigned)((N + 255) / 256);
    const unsigned n_rb = (unsigned)((M + kImRowsPerBlock - 1) / kImRowsPerBlock);
    int rc = inet_prep(c, d_src, view_stride, px_stride, px_stride == 3, nb, c->im_xs, d_bank_of, 0, 1);
    if (rc) return rc;
    hipLaunchKernelGGL(k_inet_gemv, dim3(row_blocks, (unsigned)B), dim3(256), 0, c->stream, c->im_xs, N, desc, d_tab, d_idx);
    HIP_TRY(c, hipGetLastError());
    for (int s = 0; s < steps; ++s) {
        hipLaunchKernelGGL(k_inet_upart, dim3(col_blocks, n_rb, (unsigned)B), dim3(256), 0, c->stream, N, s & 1, hs, desc, d_tab, s);
        hipLaunchKernelGGL(k_inet_ureduce, dim3(col_blocks, (unsigned)B), dim3(256), 0, c->stream, N, c->im_ku, desc, d_tab, s);
        hipLaunchKernelGGL(k_inet_update, dim3(row_blocks, (unsigned)B), dim3(256), 0, c->stream, N, s & 1, hs, c->im_ku, c->im_xs, desc, d_tab, d_idx, s);
        HIP_TRY(c, hipGetLastError());
    }
    return DV_OK;
}

// Every bank's im_flag word from its own weights (the caller has zeroed the words and reads them).
static int inet_finite(dv_ctx* c) {
    const long long n = (long long)c->inet_max_M * c->im_N, blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_inet_finite, dim3((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)c->im_banks), dim3(256), 0, c->stream,
                       c->inet_desc.device<dv::InetBank>(), c->im_N, c->im_flag);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// ibank_batch's scoring launch under a live table: nk column blocks from d_blocks on, the first of them at column c0 of X.
static int inet_score(dv_ctx* c, const dv::ImBlock* d_blocks, size_t nk, long long c0, long long cpad) {
    const dim3 grid((unsigned)((c->inet_max_M + 15) / 16), (unsigned)nk);
    const dv::InetBank* desc = c->inet_desc.device<dv::InetBank>();
    if (c->im_N % 4 == 0)
        hipLaunchKernelGGL((k_inet_score_cols<true>), grid, dim3(kImScoreWaves * 64), 0, c->stream, c->im_bx, c->im_N, desc, d_blocks, (int)c0, cpad,
                           c->im_bdpart);
    else
        hipLaunchKernelGGL((k_inet_score_cols<false>), grid, dim3(kImScoreWaves * 64), 0, c->stream, c->im_bx, c->im_N, desc, d_blocks, (int)c0, cpad,
                           c->im_bdpart);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

static int inet_decide(dv_ctx* c, int n_agents, long long cpad, int A, const int* perr, const int* d_mem, const int* d_bank_of, double* d_fam, int* d_best,
                       unsigned* d_flags) {
    hipLaunchKernelGGL(k_inet_decide, dim3((unsigned)n_agents), dim3(256), 0, c->stream, c->im_bdpart, cpad, A, perr, d_mem, d_bank_of,
                       c->inet_desc.device<dv::InetBank>(), d_fam, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

extern "C" int dv_inet_set(dv_ctx* c, int n_nets, const int32_t* n_hidden, const double* learning_rate, const int32_t* channel, const double* w0_concat,
                           int n_banks, const int32_t* network_of_bank) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need(c, "dv_inet_set");
    if (rc) return rc;
    if (!n_hidden || !learning_rate || !channel || !w0_concat) return fail(c, DV_ERR_INVALID, "dv_inet_set: NULL argument");
    if (n_nets < 1 || n_banks < 1) return fail(c, DV_ERR_INVALID, "dv_inet_set: n_nets %d or n_banks %d < 1", n_nets, n_banks);
    if (n_banks > kImMaxBanks) return fail(c, DV_ERR_INVALID, "dv_inet_set: n_banks %d outside [1, %d]", n_banks, kImMaxBanks);
    const size_t P = (size_t)n_nets, B = (size_t)n_banks, N = (size_t)c->im_N;
    std::vector<size_t> w0_off(P + 1, 0);                     // in doubles of w0_concat
    for (size_t p = 0; p < P; ++p) {
        if (n_hidden[p] < 1 || n_hidden[p] > kImMaxPixels)
            return fail(c, DV_ERR_INVALID, "dv_inet_set: network %zu: n_hidden %d outside [1, %lld]", p, (int)n_hidden[p], kImMaxPixels);
        if (!(learning_rate[p] > 0.0) || !std::isfinite(learning_rate[p]))
            return fail(c, DV_ERR_INVALID, "dv_inet_set: network %zu: learning_rate %g must be positive", p, learning_rate[p]);
        if (channel[p] < 0 || channel[p] > 2) return fail(c, DV_ERR_INVALID, "dv_inet_set: network %zu: channel %d outside [0, 2]", p, (int)channel[p]);
        w0_off[p + 1] = w0_off[p] + (size_t)n_hidden[p] * N;
    }
    rc = index_check(c, "dv_inet_set", "network_of_bank", network_of_bank, n_banks, n_nets, "n_nets");
    if (rc) return rc;
    std::vector<size_t> row0(B + 1, 0), rb0(B + 1, 0);        // prefix sums of the banks' M and of their row blocks
    int max_M = 1;
    for (size_t b = 0; b < B; ++b) {
        const size_t M = (size_t)n_hidden[network_of_bank[b]];
        row0[b + 1] = row0[b] + M;
        rb0[b + 1] = rb0[b] + (M + kImRowsPerBlock - 1) / kImRowsPerBlock;
        if ((int)M > max_M) max_M = (int)M;
    }

    HIP_TRY(c, hipSetDevice(c->device));
    double* W = nullptr, *h = nullptr, *u = nullptr, *upart = nullptr;
    int* flag = nullptr;
    MirroredTable desc;                                       // installed only when everything below has succeeded
    hipError_t e = hipMalloc((void**)&W, row0[B] * N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h, 2 * row0[B] * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&u, B * N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&upart, rb0[B] * N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&flag, B * sizeof(int));
    int up = DV_OK;                                           // table_upload's answer (it has said why)
    if (e == hipSuccess) {
        std::vector<dv::InetBank> banks(B);
        for (size_t b = 0; b < B; ++b) {
            const size_t p = (size_t)network_of_bank[b];
            banks[b] = dv::InetBank{(double DV_INET_GLOBAL*)(W + row0[b] * N), (double DV_INET_GLOBAL*)(h + row0[b]),
                                    (double DV_INET_GLOBAL*)(upart + rb0[b] * N), learning_rate[p] / (double)c->im_N, (int)n_hidden[p],
                                    (int)(rb0[b + 1] - rb0[b]), (int)channel[p], 0};
        }
        up = table_upload(c, desc, banks.data(), B * sizeof(dv::InetBank));
    }
    for (size_t b = 0; b < B && e == hipSuccess && !up; ++b) {
        const size_t p = (size_t)network_of_bank[b];
        e = hipMemcpyAsync(W + row0[b] * N, w0_concat + w0_off[p], (size_t)n_hidden[p] * N * sizeof(double), hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // `w0_concat` is borrowed for this call only; nothing enqueued reads the old weights any more
    if (e != hipSuccess || up) {                                        // the model, its banks and an earlier table stay as they were
        (void)hipGetLastError();
        auto F = [](auto* p) { if (p) (void)hipFree(p); };
        F(W); F(h); F(u); F(upart); F(flag);
        table_free(desc);
        if (up) return up;
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_inet_set: %d networks, %d banks: %s", n_nets, n_banks, hipGetErrorString(e));
    }
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->im_W); F(c->im_flag); F(c->im_kh[0]); F(c->im_kh[1]); F(c->im_ku); F(c->im_kupart);
    inet_drop(c);
    c->im_W = W;
    c->im_flag = flag;
    c->im_kh[0] = h;                                          // (both h: the second inet_h_stride doubles on; im_kh[1] stays NULL)
    c->im_ku = u;
    c->im_kupart = upart;
    c->im_banks = n_banks;
    c->im_views.assign(B, 0);
    c->im_finite.assign(B, 1);
    c->inet_desc = desc;
    c->inet_nets = n_nets;
    c->inet_max_M = max_M;
    c->inet_h_stride = row0[B];
    c->inet_M.assign(n_hidden, n_hidden + P);
    c->inet_channel.assign(channel, channel + P);
    c->inet_eta.assign(learning_rate, learning_rate + P);
    c->inet_of_bank.assign(network_of_bank, network_of_bank + B);
    c->inet_row0 = row0;
    c->inet_bytes = (row0[B] * N + 2 * row0[B] + B * N + rb0[B] * N) * sizeof(double) + B * sizeof(int) + B * sizeof(dv::InetBank);
    return ibank_check_finite(c);
}

extern "C" int dv_inet_clear(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    int rc = infomax_need(c, "dv_inet_clear");
    if (rc) return rc;
    return dv_ibank_set(c, 1, c->im_w0.data());               // one bank of the begin's network at its W0; drops the table
}

extern "C" int dv_inet_info(dv_ctx* c, int* n_nets, int* n_banks, int32_t* n_hidden, double* learning_rate, int32_t* channel, int32_t* network_of_bank,
                            int64_t* views_trained, int32_t* finite, int64_t* bytes) {
    if (!c) return DV_ERR_INVALID;
    if (n_nets) *n_nets = c->inet_nets;
    if (n_banks) *n_banks = c->inet_nets ? c->im_banks : 0;
    if (bytes) *bytes = (int64_t)c->inet_bytes;
    if (!c->inet_nets) return DV_OK;
    for (size_t p = 0; p < (size_t)c->inet_nets; ++p) {
        if (n_hidden) n_hidden[p] = c->inet_M[p];
        if (learning_rate) learning_rate[p] = c->inet_eta[p];
        if (channel) channel[p] = c->inet_channel[p];
    }
    for (size_t b = 0; b < (size_t)c->im_banks; ++b) {
        if (network_of_bank) network_of_bank[b] = c->inet_of_bank[b];
        if (views_trained) views_trained[b] = c->im_views[b];
        if (finite) finite[b] = c->im_finite[b] ? 1 : 0;
    }
    return DV_OK;
}
