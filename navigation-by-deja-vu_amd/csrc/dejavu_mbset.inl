// Mushroom-body bank sets (include/dejavu.h: dv_mbset_*): a member of a step is read out through S <= DV_MBSET_MAX_BANKS banks from ONE
// selection of firing cells.  The selection (two passes of fan_in byte gathers per cell, the histogram, the rank rule) depends on the
// view and the wiring only, so where banks share the begin's population it is done once per column, and pass 2 adds one byte per
// firing cell and bank:
//   d_j = #{k fired : wt[banks[i][j]][k] == 1},   v = sum_j coefs[i][j] d_j,   angle_fam[i][a] = (double)(-v)
// Integers throughout; the host refuses a member whose sum_j |coefs[i][j]| n_active does not fit an int32, so v cannot wrap.
//
//   k_mbset<SRC>     mb_view<kMbSet> (dejavu_mushroom.inl) on the column's plane: one statement of the selection, the read-out of its
//                    pass 2 being the set's.  SRC names the plane's source, the ones mb_batch chooses among: staged bytes (uploaded
//                    planes), the context's one landscape, a landscape set, that set under its sensor table, and both of those under
//                    noise rows.  One template over the fill: the landscape, sensor and noise-row lookups are `if constexpr` on SRC's
//                    bits.  The S bank pointers are read once per workgroup from banks[(col0 + blockIdx.x) / A] -- the CALL's column,
//                    not the launch's -- and are the same for every thread; the S accumulators are unrolled over DV_MBSET_MAX_BANKS
//                    under a uniform predicate, so they stay in registers.  Writes d[column][S].
//   k_mbset_decide   one workgroup per member: v from d and the member's coefficients, fam, the first maximum over any number of
//                    headings (mb_decide_member, k_mb_decide_batch's) and the flag.
//
// The dynamic LDS is mb_lds_bytes plus [kMbWaves][DV_MBSET_MAX_BANKS] words of wave totals; the cap is set per function, to the most
// any model can ask for (as for k_mb*: the cap is the function's, not the context's).
//
// Not built: sets across populations (banks of different populations share no selection: the calls are refused while a population
// table is live), coefficients that are not integers, multi-device forms.
namespace dv {

static constexpr int kSetStaged = 0, kSetPose = 1, kSetLands = 2, kSetSensors = 4, kSetNoise = 8;

// Where a column's plane comes from; which members are read depends on SRC.
struct MbSetSrc {
    const unsigned char* bytes;      // staged planes uint8[columns][N] | the context's landscape | the set's landscapes
    const LandEntry* tab;            // kSetLands
    const SensorEntry* sens;         // kSetSensors
    const unsigned char* lut;        // the context's level table | kSetSensors: the table's, 768 bytes per landscape
    const int* land_of;              // kSetLands: the call's table, a landscape per member
    const NoiseRow* rows;            // kSetNoise: a row per member
    const Pose* poses;               // kSetPose: from this launch's first column on
    int* err;                        // kSetPose: a word per column, from this launch's first column on
    SensorCfg g;
    int channel;
};

// d: from this launch's first column on; banks: the whole call's [members][S]; col0: the launch's first column within the call.
template <int SRC>
__global__ __launch_bounds__(kMbWaves * 64) void k_mbset(MbSetSrc s, int N, const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                         const unsigned char* __restrict__ wt, int* __restrict__ d,
                                                         const int* __restrict__ banks, int S, unsigned col0, unsigned A) {
    extern __shared__ unsigned mb_lds[];
    const unsigned col = col0 + blockIdx.x;
    const int* mine = banks + (size_t)(col / A) * (size_t)S;
    MbSetWts set;
    set.S = S;
#pragma unroll
    for (int j = 0; j < kMbSetMax; ++j) set.w[j] = wt + (size_t)mine[j < S ? j : 0] * (size_t)K;
    if constexpr (SRC == kSetStaged) {
        mb_view<kMbSet>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_staged(plane, tid, s.bytes, (long long)N, 1, 0, N); },
                        (int)blockIdx.x, N, conn, K, c, n_active, nullptr, d, nullptr, nullptr, set);
    } else {
        constexpr bool NOISE = (SRC & kSetNoise) != 0;
        SensorCfg g = s.g;
        const unsigned char* lut = s.lut;
        const unsigned char* land = s.bytes;
        if constexpr ((SRC & kSetSensors) != 0) land = land_sensor_of_column(s.bytes, s.tab, s.sens, s.lut, s.land_of, col, A, g, lut);
        else if constexpr ((SRC & kSetLands) != 0) land = land_of_column(s.bytes, s.tab, s.land_of, col, A, g);
        const NoiseRow* row = NOISE ? s.rows + col / A : nullptr;
        const unsigned long long a_N = NOISE ? (unsigned long long)(col % A) * (unsigned)N : 0ull;
        mb_view<kMbSet>(mb_lds,
                        [&](unsigned char* plane, int tid) { mb_fill_pose<NOISE>(plane, tid, land, s.poses, g, lut, s.channel, N, s.err, row, a_N); },
                        (int)blockIdx.x, N, conn, K, c, n_active, nullptr, d, nullptr, nullptr, set);
    }
}

// One workgroup per member i: v[a] = sum_j coefs[i][j] d[i A + a][j], fam[i A + a] = (double)(-v[a]), the first maximum of fam and the
// member's flag (perr as k_mb_decide_batch's).  |v| fits an int32: the host has checked sum_j |coefs[i][j]| n_active.
__global__ __launch_bounds__(256) void k_mbset_decide(const int* __restrict__ d, const int* __restrict__ coefs, int S, const int* __restrict__ perr,
                                                      int A, double* __restrict__ fam, int* __restrict__ best, unsigned* __restrict__ flags) {
    const int tid = (int)threadIdx.x;
    const size_t col0 = (size_t)blockIdx.x * (size_t)A;
    const int* cf = coefs + (size_t)blockIdx.x * (size_t)S;
    int bv = 0, bi = -1, bad = 0;
    for (int a = tid; a < A; a += 256) {                      // headings in rising order: a later equal does not replace
        const int* dc = d + (col0 + a) * (size_t)S;
        int v = 0;
        for (int j = 0; j < S; ++j) v -= cf[j] * dc[j];
        fam[col0 + a] = (double)v;
        if (bi < 0 || v > bv) { bv = v; bi = a; }
        if (perr) bad |= perr[col0 + a];
    }
    mb_decide_member(bv, bi, bad, best, flags);
}

}  // namespace dv

static size_t mbset_lds_bytes(int N, int fan_in) { return mb_lds_bytes(N, fan_in) + (size_t)kMbWaves * (size_t)kMbSetMax * 4u; }

static void mbset_free(dv_ctx* c) {
    if (c->mbs_d) { (void)hipFree(c->mbs_d); c->mbs_d = nullptr; }
    c->mbs_d_cap = 0;
    table_free(c->mbs_banks);
    table_free(c->mbs_coefs);
}

// The cap on dynamic LDS of every k_mbset form: this family's own maximum, whatever the context's model needs (dv_mb_begin).
static hipError_t mbset_lds_cap() {
    const int lds = (int)mbset_lds_bytes(kMbMaxPixels, dv::kMbMaxFanIn);
    hipError_t e = hipFuncSetAttribute((const void*)k_mbset<kSetStaged>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mbset<kSetPose>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mbset<kSetPose | kSetLands>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_mbset<kSetPose | kSetLands | kSetSensors>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_mbset<kSetPose | kSetLands | kSetNoise>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_mbset<kSetPose | kSetLands | kSetSensors | kSetNoise>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
}

template <int SRC>
static int mbset_launch(dv_ctx* c, const MbSetSrc& s, int nc, int* d, int S, long long c0, int A) {
    hipLaunchKernelGGL((k_mbset<SRC>), dim3((unsigned)nc), dim3(kMbWaves * 64), mbset_lds_bytes(c->mb_N, c->mb_c), c->stream, s, c->mb_N, c->mb_conn,
                       c->mb_K, c->mb_c, c->mb_active, c->mb_wt, d, c->mbs_banks.device<int>(), S, (unsigned)c0, (unsigned)A);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// The three calls' one path, mb_batch's shape: every table checked entry by entry before anything reaches the device, tables uploaded
// only when the device does not hold them already, launches of at most kMbSlabViews (or mb_slab(N) uploaded) columns one after another
// on the stream, one wait.  planes != nullptr: uploaded uint8[n_agents][A][h][w]; else the poses, on the context's landscape
// (land_of == nullptr) or on landscape land_of[i] of the set, under the set's sensor table and live noise rows where there are any.
static int mbset_batch(dv_ctx* c, const char* who, const uint8_t* planes, const double* x, const double* y, const double* angles, int n_agents, int A,
                       int S, const int32_t* banks, const int32_t* coefs, const int32_t* land_of, bool with_lands, double* angle_fam,
                       int32_t* best_heading, uint32_t* flags, int32_t* bank_novelty) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, who);
    if (rc) return rc;
    if (c->mbp_pops)
        return fail(c, DV_ERR_STATE, "%s: a population table is live, and banks of different populations share no selection (not built; dv_mbpop_clear first)", who);
    if (S < 1 || S > DV_MBSET_MAX_BANKS) return fail(c, DV_ERR_INVALID, "%s: set_size %d outside [1, DV_MBSET_MAX_BANKS = %d]", who, S, DV_MBSET_MAX_BANKS);
    const bool sensed = planes == nullptr;
    if ((sensed ? (!x || !y || !angles || !flags) : false) || !banks || !coefs || !angle_fam || !best_heading || n_agents < 1 || A < 1 ||
        (with_lands && !land_of))
        return fail(c, DV_ERR_INVALID, "%s: NULL argument, n_agents < 1 or n_headings < 1", who);
    if (sensed) { rc = sensor_fits(c, who, c->mb_hh, c->mb_ww); if (rc) return rc; }
    const long long C = (long long)n_agents * A;
    if (C * S > 0x7fffffffll) return fail(c, DV_ERR_INVALID, "%s: %d agents x %d headings x %d banks are too many values", who, n_agents, A, S);
    for (int i = 0; i < n_agents; ++i) {
        long long mag = 0;
        for (int j = 0; j < S; ++j) {
            const int32_t b = banks[(size_t)i * S + j];
            if (b < 0 || b >= c->mb_banks)
                return fail(c, DV_ERR_INVALID, "%s: banks[%d][%d] = %d outside [0, n_banks = %d)", who, i, j, (int)b, c->mb_banks);
            const long long cf = coefs[(size_t)i * S + j];
            mag += cf < 0 ? -cf : cf;
        }
        if (mag * c->mb_active > 0x7fffffffll)
            return fail(c, DV_ERR_INVALID, "%s: member %d: sum |coefs| = %lld times n_active = %d exceeds 2^31 - 1", who, i, mag, c->mb_active);
    }
    if (land_of) { rc = lands_check(c, who, "land_of_member", land_of, n_agents); if (rc) return rc; }
    else if (sensed) { rc = noise_need_lands(c, who); if (rc) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->mb_N;
    long long slab = planes ? (long long)mb_slab(N) : (long long)kMbSlabViews;
    if (slab > C) slab = C;
    double* d_fam = nullptr; int* d_best = nullptr; unsigned* d_flags = nullptr;   // the packed results' parts on the device
    rc = grow_buffer(c, c->mbs_d, c->mbs_d_cap, (size_t)C * (size_t)S * sizeof(int));
    if (!rc) rc = packed_device(c, c->mb_res, C, n_agents, d_fam, d_best, d_flags);
    if (!rc && sensed) rc = grow_buffer(c, c->mb_berr, c->mb_berr_cap, (size_t)C * sizeof(int));
    if (!rc && planes) rc = ensure_sense_buffer(c, (size_t)slab * N);
    if (!rc) rc = table_upload(c, c->mbs_banks, banks, (size_t)n_agents * (size_t)S * sizeof(int));
    if (!rc) rc = table_upload(c, c->mbs_coefs, coefs, (size_t)n_agents * (size_t)S * sizeof(int));
    if (!rc && land_of) rc = lands_upload(c, land_of, n_agents);
    if (!rc && sensed) rc = upload_member_poses(c, x, y, angles, n_agents, A);
    if (rc) return rc;
    for (long long c0 = 0; c0 < C; c0 += slab) {
        const int nc = (int)(C - c0 < slab ? C - c0 : slab);
        int* d = c->mbs_d + (size_t)c0 * (size_t)S;
        MbSetSrc s{};
        s.g = c->sensor;
        s.channel = c->mb_channel;
        if (planes) {
            HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)c0 * N, (size_t)nc * N, hipMemcpyHostToDevice, c->stream));
            s.bytes = c->d_sense;
            rc = mbset_launch<kSetStaged>(c, s, nc, d, S, c0, A);
        } else {
            s.poses = c->d_poses + c0;
            s.err = c->mb_berr + c0;
            s.lut = c->d_lut;
            if (!land_of) {
                s.bytes = c->d_land;
                rc = mbset_launch<kSetPose>(c, s, nc, d, S, c0, A);
            } else {
                s.bytes = c->ld_lands;
                s.tab = c->ld_tab;
                s.land_of = c->ld_of.device<int>();
                if (c->nz_n) s.rows = c->nz_tab.device<NoiseRow>();   // (uploaded beside the landscape table, dejavu_noise.inl)
                if (c->sn_tab) { s.sens = c->sn_tab; s.lut = c->sn_luts; }
                if (c->nz_n && c->sn_tab) rc = mbset_launch<kSetPose | kSetLands | kSetSensors | kSetNoise>(c, s, nc, d, S, c0, A);
                else if (c->nz_n) rc = mbset_launch<kSetPose | kSetLands | kSetNoise>(c, s, nc, d, S, c0, A);
                else if (c->sn_tab) rc = mbset_launch<kSetPose | kSetLands | kSetSensors>(c, s, nc, d, S, c0, A);
                else rc = mbset_launch<kSetPose | kSetLands>(c, s, nc, d, S, c0, A);
            }
        }
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_mbset_decide, dim3((unsigned)n_agents), dim3(256), 0, c->stream, c->mbs_d, c->mbs_coefs.device<int>(), S,
                       planes ? nullptr : c->mb_berr, A, d_fam, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    rc = packed_fetch(c, c->mb_res, C, n_agents);
    if (rc) return rc;
    if (bank_novelty) HIP_TRY(c, hipMemcpyAsync(bank_novelty, c->mbs_d, (size_t)C * (size_t)S * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    packed_unpack(c->mb_res, C, n_agents, angle_fam, best_heading, flags);
    return DV_OK;
}

extern "C" int dv_mbset_step_u8(dv_ctx* c, const uint8_t* planes, int n_agents, int n_headings, int set_size, const int32_t* banks,
                                const int32_t* coefs, double* angle_fam, int32_t* best_heading, int32_t* bank_novelty) {
    if (!c) return DV_ERR_INVALID;
    if (!planes) return fail(c, DV_ERR_INVALID, "dv_mbset_step_u8: planes is NULL");
    return mbset_batch(c, "dv_mbset_step_u8", planes, nullptr, nullptr, nullptr, n_agents, n_headings, set_size, banks, coefs, nullptr, false, angle_fam,
                       best_heading, nullptr, bank_novelty);
}

extern "C" int dv_mbset_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings, int set_size,
                                   const int32_t* banks, const int32_t* coefs, double* angle_fam, int32_t* best_heading, uint32_t* flags,
                                   int32_t* bank_novelty) {
    return mbset_batch(c, "dv_mbset_sense_step", nullptr, x, y, angles, n_agents, n_headings, set_size, banks, coefs, nullptr, false, angle_fam,
                       best_heading, flags, bank_novelty);
}

extern "C" int dv_mbset_lands_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings, int set_size,
                                         const int32_t* banks, const int32_t* coefs, const int32_t* land_of_member, double* angle_fam,
                                         int32_t* best_heading, uint32_t* flags, int32_t* bank_novelty) {
    return mbset_batch(c, "dv_mbset_lands_sense_step", nullptr, x, y, angles, n_agents, n_headings, set_size, banks, coefs, land_of_member, true,
                       angle_fam, best_heading, flags, bank_novelty);
}
