// Population tables of the mushroom-body model (include/dejavu.h: dv_mbpop_*): a memory bank with cells, wiring, quota and compared
// channel of its own.  A population is (channel, K = n_kc, c = fan_in, n_active, conn uint16[c][K]); the table gives the engine P
// populations and B banks, population_of_bank[b] naming bank b's.  The views' h x w, so N, stay the ones dv_mb_begin fixed.
//
// The device keeps one descriptor per BANK (MbPopBank: its population's connectivity, its own weights, K, c, n_active, channel), so a
// workgroup reads two words more than k_mb_bank's: its column's bank, bank_of[(col0 + blockIdx.x) / per] -- the CALL's column, as
// mb_bank reads it -- and then that bank's descriptor.  Both are the same for every lane of the workgroup, so they are scalar loads.
// Everything after them is mb_view<MODE> (dejavu_mushroom.inl) on the descriptor's values: the span of a wave, nb = 255 c + 1 and the
// place of the hand-over words in LDS follow the bank's own K and c because mb_view computes them from its arguments.
//
//   k_mbpop_bank<kMbTrain | kMbScore>   k_mb_bank on a bank's own population.  by_channel: the source is the sensed uint8[n][h][w][3]
//                (training from poses), read at the bank's channel; else the staged bytes are the compared plane already.
//   k_mbpop_pose_bank, k_mbpop_pose_bank_lands, k_mbpop_pose_bank_lands_sensors   k_mb_pose_bank and its landscape-set forms:
//                mb_fill_pose picks the bank's byte of every sensed pixel.
//   k_mbpop_count   k_mb_count over ragged banks: one workgroup per bank, the bank's own length.
//
// Weights are ragged: uint8, bank b at the sum of its predecessors' K, no padding.  Training views of many banks and populations in one
// launch is safe for the reason it is without a table: every writer of a byte stores 0, and a workgroup writes inside its own bank
// only (wt + k, k < its K); nothing is atomic outside the LDS histogram.  A launch's dynamic LDS is the most any population of the
// table asks for, mb_lds_bytes(N, max c); a workgroup uses the first mb_lds_bytes(N, c of its bank) of it.
namespace dv {

// A pointer read from memory is a flat one to the compiler, and a flat load counts on the LDS counter as well as on the memory
// counter, so mb_activity's index loads would queue with the plane's gathers (measured: +19 us on a 140 us step).  The descriptor's
// pointers are therefore typed as what they are, global memory; cast to the plain pointers mb_view takes, they give the global loads
// and stores a kernel argument gets.
#define DV_MBPOP_GLOBAL __attribute__((address_space(1)))

struct MbPopBank {
    const unsigned short DV_MBPOP_GLOBAL* conn;   // [c][K] of the bank's population
    unsigned char DV_MBPOP_GLOBAL* wt;            // [K]: the bank's own weights
    int K, c, n_active, channel;
};

// The descriptor of workgroup blockIdx.x's bank (the host has checked the bank table against [0, n_banks), and the descriptor table
// holds n_banks entries).
__device__ __forceinline__ MbPopBank mbpop_bank(const MbPopBank* __restrict__ desc, const int* __restrict__ bank_of, unsigned col0, unsigned per) {
    return desc[bank_of[(col0 + blockIdx.x) / per]];
}

template <int MODE>
__global__ __launch_bounds__(kMbWaves * 64) void k_mbpop_bank(const unsigned char* __restrict__ src, long long view_stride, int px_stride, int by_channel,
                                                              int N, const MbPopBank* __restrict__ desc, int* __restrict__ d,
                                                              const int* __restrict__ bank_of, unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const MbPopBank b = mbpop_bank(desc, bank_of, col0, per);
    const int offset = by_channel ? b.channel : 0;
    mb_view<MODE>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_staged(plane, tid, src, view_stride, px_stride, offset, N); },
                  (int)blockIdx.x, N, (const unsigned short*)b.conn, b.K, b.c, b.n_active, (unsigned char*)b.wt, d, nullptr, nullptr);
}

__global__ __launch_bounds__(kMbWaves * 64) void k_mbpop_pose_bank(const unsigned char* __restrict__ land, const Pose* __restrict__ poses, SensorCfg g,
                                                                   const unsigned char* __restrict__ lut, const MbPopBank* __restrict__ desc,
                                                                   int* __restrict__ d, int* __restrict__ err, const int* __restrict__ bank_of,
                                                                   unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    const MbPopBank b = mbpop_bank(desc, bank_of, col0, per);
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose(plane, tid, land, poses, g, lut, b.channel, N, err); },
                      (int)blockIdx.x, N, (const unsigned short*)b.conn, b.K, b.c, b.n_active, (unsigned char*)b.wt, d, nullptr, nullptr);
}

__global__ __launch_bounds__(kMbWaves * 64) void k_mbpop_pose_bank_lands(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                                                         const int* __restrict__ land_of, const Pose* __restrict__ poses, SensorCfg g,
                                                                         const unsigned char* __restrict__ lut, const MbPopBank* __restrict__ desc,
                                                                         int* __restrict__ d, int* __restrict__ err, const int* __restrict__ bank_of,
                                                                         unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    const unsigned char* land = land_of_column(lands, tab, land_of, col0 + blockIdx.x, per, g);
    const MbPopBank b = mbpop_bank(desc, bank_of, col0, per);
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose(plane, tid, land, poses, g, lut, b.channel, N, err); },
                      (int)blockIdx.x, N, (const unsigned short*)b.conn, b.K, b.c, b.n_active, (unsigned char*)b.wt, d, nullptr, nullptr);
}

__global__ __launch_bounds__(kMbWaves * 64) void k_mbpop_pose_bank_lands_sensors(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                                                                 const SensorEntry* __restrict__ sens,
                                                                                 const unsigned char* __restrict__ luts, const int* __restrict__ land_of,
                                                                                 const Pose* __restrict__ poses, SensorCfg g,
                                                                                 const MbPopBank* __restrict__ desc, int* __restrict__ d,
                                                                                 int* __restrict__ err, const int* __restrict__ bank_of, unsigned col0,
                                                                                 unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    const unsigned char* lut;
    const unsigned char* land = land_sensor_of_column(lands, tab, sens, luts, land_of, col0 + blockIdx.x, per, g, lut);
    const MbPopBank b = mbpop_bank(desc, bank_of, col0, per);
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose(plane, tid, land, poses, g, lut, b.channel, N, err); },
                      (int)blockIdx.x, N, (const unsigned short*)b.conn, b.K, b.c, b.n_active, (unsigned char*)b.wt, d, nullptr, nullptr);
}

// zeros[b] = the zero weights of bank b = blockIdx.x, over the K of its own population.
__global__ __launch_bounds__(256) void k_mbpop_count(const MbPopBank* __restrict__ desc, long long* __restrict__ zeros) {
    __shared__ int red[256];
    const int tid = (int)threadIdx.x;
    const unsigned char DV_MBPOP_GLOBAL* wt = desc[blockIdx.x].wt;
    const int K = desc[blockIdx.x].K;
    int s = 0;
    for (int k = tid; k < K; k += 256) s += wt[k] == 0 ? 1 : 0;
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) zeros[blockIdx.x] = (long long)red[0];
}

}  // namespace dv

// The function-wide cap on dynamic LDS of the kernels above (dv_mb_begin sets it with k_mb*'s, for the reason it gives there).
static hipError_t mbpop_lds_cap(int lds) {
    hipError_t e = hipFuncSetAttribute((const void*)k_mbpop_bank<kMbTrain>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mbpop_bank<kMbScore>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mbpop_pose_bank, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mbpop_pose_bank_lands, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mbpop_pose_bank_lands_sensors, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

// Forget the table (not the weights: the caller replaces or frees those).
static void mbpop_drop(dv_ctx* c) {
    if (c->mbp_conn) { (void)hipFree(c->mbp_conn); c->mbp_conn = nullptr; }
    table_free(c->mbp_desc);
    c->mbp_pops = 0;
    c->mbp_lds = c->mbp_bytes = 0;
    c->mbp_K.clear(); c->mbp_c.clear(); c->mbp_active.clear(); c->mbp_channel.clear(); c->mbp_of_bank.clear(); c->mbp_wt_off.clear();
}

// mb_launch_bank under a live table: view v of the launch works through the population of bank d_bank_of[(col0 + v) / per].
static int mbpop_launch_bank(dv_ctx* c, int mode, const unsigned char* d_src, long long view_stride, int px_stride, int by_channel, int n, int* d,
                             const int* d_bank_of, long long col0, int per) {
    const dv::MbPopBank* desc = c->mbp_desc.device<dv::MbPopBank>();
    if (mode == kMbTrain)
        hipLaunchKernelGGL((k_mbpop_bank<kMbTrain>), dim3((unsigned)n), dim3(kMbWaves * 64), c->mbp_lds, c->stream, d_src, view_stride, px_stride,
                           by_channel, c->mb_N, desc, d, d_bank_of, (unsigned)col0, (unsigned)per);
    else
        hipLaunchKernelGGL((k_mbpop_bank<kMbScore>), dim3((unsigned)n), dim3(kMbWaves * 64), c->mbp_lds, c->stream, d_src, view_stride, px_stride,
                           by_channel, c->mb_N, desc, d, d_bank_of, (unsigned)col0, (unsigned)per);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// mb_batch's sensed launch under a live table: nc columns from column c0 of the call on, A columns a member; on_lands: the members'
// landscapes are in c->ld_of (and their sensors in the set's sensor table, where it has one).
static int mbpop_launch_pose(dv_ctx* c, bool on_lands, long long c0, int nc, int A) {
    const dv::MbPopBank* desc = c->mbp_desc.device<dv::MbPopBank>();
    const int* bank_of = c->mb_bank_of.device<int>();
    if (on_lands && c->sn_tab)
        hipLaunchKernelGGL(k_mbpop_pose_bank_lands_sensors, dim3((unsigned)nc), dim3(kMbWaves * 64), c->mbp_lds, c->stream, c->ld_lands, c->ld_tab, c->sn_tab,
                           c->sn_luts, c->ld_of.device<int>(), c->d_poses + c0, c->sensor, desc, c->mb_bd + c0, c->mb_berr + c0, bank_of, (unsigned)c0,
                           (unsigned)A);
    else if (on_lands)
        hipLaunchKernelGGL(k_mbpop_pose_bank_lands, dim3((unsigned)nc), dim3(kMbWaves * 64), c->mbp_lds, c->stream, c->ld_lands, c->ld_tab,
                           c->ld_of.device<int>(), c->d_poses + c0, c->sensor, c->d_lut, desc, c->mb_bd + c0, c->mb_berr + c0, bank_of, (unsigned)c0,
                           (unsigned)A);
    else
        hipLaunchKernelGGL(k_mbpop_pose_bank, dim3((unsigned)nc), dim3(kMbWaves * 64), c->mbp_lds, c->stream, c->d_land, c->d_poses + c0, c->sensor, c->d_lut,
                           desc, c->mb_bd + c0, c->mb_berr + c0, bank_of, (unsigned)c0, (unsigned)A);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// Enqueue the zero weights of every bank into c->mb_zeros.
static int mbpop_count(dv_ctx* c) {
    hipLaunchKernelGGL(k_mbpop_count, dim3((unsigned)c->mb_banks), dim3(256), 0, c->stream, c->mbp_desc.device<dv::MbPopBank>(), c->mb_zeros);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

extern "C" int dv_mbpop_set(dv_ctx* c, int n_pops, const int32_t* n_kc, const int32_t* fan_in, const int32_t* n_active, const int32_t* channel,
                            const int32_t* conn_concat, int n_banks, const int32_t* population_of_bank) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_mbpop_set");
    if (rc) return rc;
    if (!n_kc || !fan_in || !n_active || !channel || !conn_concat) return fail(c, DV_ERR_INVALID, "dv_mbpop_set: NULL argument");
    if (n_pops < 1 || n_banks < 1) return fail(c, DV_ERR_INVALID, "dv_mbpop_set: n_pops %d or n_banks %d < 1", n_pops, n_banks);
    const size_t P = (size_t)n_pops, B = (size_t)n_banks;
    const int N = c->mb_N;
    std::vector<size_t> conn_off(P + 1, 0);                   // in uint16 words of the device's layout (the caller's int32 alike)
    int max_c = 1;
    for (size_t p = 0; p < P; ++p) {
        if (n_kc[p] < 1 || n_kc[p] > kMbMaxCells) return fail(c, DV_ERR_INVALID, "dv_mbpop_set: population %zu: n_kc %d outside [1, %d]", p, (int)n_kc[p], kMbMaxCells);
        if (fan_in[p] < 1 || fan_in[p] > dv::kMbMaxFanIn)
            return fail(c, DV_ERR_INVALID, "dv_mbpop_set: population %zu: fan_in %d outside [1, %d]", p, (int)fan_in[p], dv::kMbMaxFanIn);
        if (n_active[p] < 1 || n_active[p] > n_kc[p])
            return fail(c, DV_ERR_INVALID, "dv_mbpop_set: population %zu: n_active %d outside [1, n_kc = %d]", p, (int)n_active[p], (int)n_kc[p]);
        if (channel[p] < 0 || channel[p] > 2) return fail(c, DV_ERR_INVALID, "dv_mbpop_set: population %zu: channel %d outside [0, 2]", p, (int)channel[p]);
        conn_off[p + 1] = conn_off[p] + (size_t)n_kc[p] * (size_t)fan_in[p];
        if (fan_in[p] > max_c) max_c = fan_in[p];
    }
    rc = index_check(c, "dv_mbpop_set", "population_of_bank", population_of_bank, n_banks, n_pops, "n_pops");
    if (rc) return rc;
    // the device's layout of every population: uint16 [fan_in][n_kc], as dv_mb_begin's
    std::vector<unsigned short> ct(conn_off[P]);
    for (size_t p = 0; p < P; ++p) {
        const size_t K = (size_t)n_kc[p], cc = (size_t)fan_in[p];
        const int32_t* conn = conn_concat + conn_off[p];
        unsigned short* t = ct.data() + conn_off[p];
        for (size_t k = 0; k < K; ++k)
            for (size_t j = 0; j < cc; ++j) {
                const int32_t v = conn[k * cc + j];
                if (v < 0 || v >= N) return fail(c, DV_ERR_INVALID, "dv_mbpop_set: population %zu: conn[%zu][%zu] = %d outside [0, %d)", p, k, j, (int)v, N);
                t[j * K + k] = (unsigned short)v;
            }
    }
    std::vector<size_t> wt_off(B + 1, 0);
    for (size_t b = 0; b < B; ++b) wt_off[b + 1] = wt_off[b] + (size_t)n_kc[population_of_bank[b]];

    HIP_TRY(c, hipSetDevice(c->device));
    unsigned short* conn_dev = nullptr;
    unsigned char* wt = nullptr;
    long long* zeros = nullptr;
    MirroredTable desc;                                       // installed only when everything below has succeeded
    hipError_t e = hipMalloc((void**)&conn_dev, ct.size() * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMalloc((void**)&wt, wt_off[B]);
    if (e == hipSuccess) e = hipMalloc((void**)&zeros, B * sizeof(long long));
    int up = DV_OK;                                           // table_upload's answer (it has said why)
    if (e == hipSuccess) {
        std::vector<dv::MbPopBank> banks(B);
        for (size_t b = 0; b < B; ++b) {
            const size_t p = (size_t)population_of_bank[b];
            banks[b] = dv::MbPopBank{(const unsigned short DV_MBPOP_GLOBAL*)(conn_dev + conn_off[p]), (unsigned char DV_MBPOP_GLOBAL*)(wt + wt_off[b]), (int)n_kc[p], (int)fan_in[p], (int)n_active[p], (int)channel[p]};
        }
        up = table_upload(c, desc, banks.data(), B * sizeof(dv::MbPopBank));
    }
    if (e == hipSuccess && !up) e = hipMemcpyAsync(conn_dev, ct.data(), ct.size() * sizeof(unsigned short), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && !up) e = hipMemsetAsync(wt, 1, wt_off[B], c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // `ct` is this call's; nothing enqueued reads the old weights any more
    if (e != hipSuccess || up) {                                        // the model and its banks stay as they were
        (void)hipGetLastError();
        if (conn_dev) (void)hipFree(conn_dev);
        if (wt) (void)hipFree(wt);
        if (zeros) (void)hipFree(zeros);
        table_free(desc);
        if (up) return up;
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_mbpop_set: %d populations, %d banks: %s", n_pops, n_banks,
                    hipGetErrorString(e));
    }
    (void)hipFree(c->mb_wt);
    (void)hipFree(c->mb_zeros);
    mbpop_drop(c);
    c->mb_wt = wt;
    c->mb_zeros = zeros;
    c->mb_banks = n_banks;
    c->mb_views.assign(B, 0);
    c->mbp_conn = conn_dev;
    c->mbp_desc = desc;
    c->mbp_pops = n_pops;
    c->mbp_K.assign(n_kc, n_kc + P); c->mbp_c.assign(fan_in, fan_in + P); c->mbp_active.assign(n_active, n_active + P);
    c->mbp_channel.assign(channel, channel + P);
    c->mbp_of_bank.assign(population_of_bank, population_of_bank + B);
    c->mbp_wt_off = wt_off;
    c->mbp_lds = mb_lds_bytes(N, max_c);
    c->mbp_bytes = wt_off[B] + ct.size() * sizeof(unsigned short) + B * sizeof(dv::MbPopBank);
    return DV_OK;
}

extern "C" int dv_mbpop_clear(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_mbpop_clear");
    if (rc) return rc;
    return dv_mbank_set(c, 1);                                // one bank of the begin's population, weights 1; drops the table
}

extern "C" int dv_mbpop_info(dv_ctx* c, int* n_pops, int* n_banks, int32_t* n_kc, int32_t* fan_in, int32_t* n_active, int32_t* channel,
                             int32_t* population_of_bank, int64_t* views_trained, int64_t* n_depressed, int64_t* bytes) {
    if (!c) return DV_ERR_INVALID;
    if (n_pops) *n_pops = c->mbp_pops;
    if (n_banks) *n_banks = c->mbp_pops ? c->mb_banks : 0;
    if (bytes) *bytes = (int64_t)c->mbp_bytes;
    if (!c->mbp_pops) return DV_OK;
    const size_t P = (size_t)c->mbp_pops, B = (size_t)c->mb_banks;
    for (size_t p = 0; p < P; ++p) {
        if (n_kc) n_kc[p] = c->mbp_K[p];
        if (fan_in) fan_in[p] = c->mbp_c[p];
        if (n_active) n_active[p] = c->mbp_active[p];
        if (channel) channel[p] = c->mbp_channel[p];
    }
    for (size_t b = 0; b < B; ++b) {
        if (population_of_bank) population_of_bank[b] = c->mbp_of_bank[b];
        if (views_trained) views_trained[b] = c->mb_views[b];
    }
    if (n_depressed) {
        std::vector<long long> z(B);
        HIP_TRY(c, hipSetDevice(c->device));
        int rc = mbpop_count(c);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(z.data(), c->mb_zeros, B * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t b = 0; b < B; ++b) n_depressed[b] = (int64_t)z[b];
    }
    return DV_OK;
}
