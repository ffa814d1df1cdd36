// Noise rows (include/dejavu.h: dv_noise_*): sensor noise on landscape sets, a reproducible draw per sensing.  The sensed views are a
// deterministic function of the pose; with rows live, every sensed call that takes a landscape table adds to the S and V of every
// sensor pixel an integer drawn from a counter-based generator, so that two members at one pose see different bytes, a replicate
// differs from another in its draws alone, and NumPy restates every byte (tests/helpers_noise.py).
//
// The statement.  Row i = (key, amp_s, amp_v) belongs to member i of a step or scene call (per = A headings a row) or to view / pose i
// of a training, store or dv_lands_sense call (per = 1).  For sensor pixel j = bi sw + bj of the row's heading a, with P = sh sw:
//     base = splitmix64(key + seed GOLDEN)            (made on the host, once per row: NoiseRow::base)
//     word = splitmix64(base + (a P + j))             d_S = word & 0xFFFFFFFF, d_V = word >> 32
//     n_c  = ((d_c (2 amp_c + 1)) >> 32) - amp_c      an integer in [-amp_c, +amp_c]
//     S'   = clamp(S + n_S, 0, 255), V' likewise
// S and V are the pixel's values after the block rule and before the level tables (noise_apply in dejavu_kernels.h, called by
// sense_thread<EACH, true> and sense_pixel<true>); the hue is the noiseless model's, the level tables and the mask follow.  A row of
// zero amplitudes gives the noiseless bytes.  The draw depends on the row's key and the pixel's place within the member, never on the
// launch, the member's index or who else is in the call: the row and heading of a pose come from its column within the CALL,
// (col0 + pose) / per and % per, the rule land_of_column uses, so a launch that begins inside a member draws what one launch would.
//
//   k_sense_lands_noise                  k_sense_lands under the pose's row
//   k_sense_lands_sensors_noise          k_sense_lands_sensors likewise
//   k_mb_pose_bank_lands_noise / _sensors_noise   (dejavu_mushroom.inl) the mushroom body's pose kernels; a workgroup is one column, so one row
//
// The rows ride with the call's landscape table: lands_check refuses a table whose length is not the rows' (before anything reaches the
// device), lands_upload brings the device's rows up to date beside the table (table_upload: an unchanged table is not sent again), and
// the Infomax banked step, which senses in bank-sorted order, hands lands_upload its permutation.  With no rows every call launches
// exactly what it launched before there were rows: the forms above are kernels of their own, chosen on the host.
//
// Not built: hue noise; any non-uniform law; noise on the context's one landscape (calls without a landscape table are refused while
// rows are live, DV_ERR_STATE, lest they sense without noise unnoticed); the library path (dv_step*, dv_sense_step*), single agents and
// dv_sense, which stay noiseless; noise forms of the population table's pose kernels (dejavu_mbpop.inl), so the mushroom step under a
// population table is refused while rows are live (Infomax network tables sense through lands_launch_sense and are served).
namespace dv {

__global__ void k_sense_lands_noise(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab, const int* __restrict__ land_of,
                                    const NoiseRow* __restrict__ rows, unsigned col0, unsigned per, const Pose* __restrict__ poses, int n, SensorCfg g,
                                    const unsigned char* __restrict__ lut, unsigned char* __restrict__ out, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pose = t / ((long long)g.sw * g.sh);
    if (pose >= n) return;                                     // (before the tables are read)
    const unsigned char* land = land_of_column(lands, tab, land_of, col0 + (unsigned)pose, per, g);
    sense_thread<true, true>(land, poses, n, g, lut, out, err, NoiseArgs{rows, col0, per});
}

__global__ void k_sense_lands_sensors_noise(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                            const SensorEntry* __restrict__ sens, const unsigned char* __restrict__ luts,
                                            const int* __restrict__ land_of, const NoiseRow* __restrict__ rows, unsigned col0, unsigned per,
                                            const Pose* __restrict__ poses, int n, SensorCfg g, unsigned char* __restrict__ out,
                                            int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pose = t / ((long long)g.sw * g.sh);
    if (pose >= n) return;                                     // (before the tables are read)
    const unsigned char* lut;
    const unsigned char* land = land_sensor_of_column(lands, tab, sens, luts, land_of, col0 + (unsigned)pose, per, g, lut);
    sense_thread<true, true>(land, poses, n, g, lut, out, err, NoiseArgs{rows, col0, per});
}

}  // namespace dv

static void noise_drop(dv_ctx* c) {
    c->nz_n = 0;
    c->nz_seed = 0;
    c->nz_keys.clear();
    c->nz_amp_s.clear();
    c->nz_amp_v.clear();
    c->nz_rows.clear();
    c->nz_sorted.clear();
    table_free(c->nz_tab);
}

// Live rows are one per entry of a call's landscape table: a table of another length is refused before anything reaches the device.
static int noise_check(dv_ctx* c, const char* who, const char* what, int64_t n) {
    if (c->nz_n && n != c->nz_n)
        return fail(c, DV_ERR_INVALID, "%s: %s holds %lld entries, but %lld noise rows are live (dv_noise_rows sets a row per entry; dv_noise_clear drops them)",
                    who, what, (long long)n, (long long)c->nz_n);
    return DV_OK;
}

// A sensed call without a landscape table, while rows are live: refused, since it would sense without noise.
static int noise_need_lands(dv_ctx* c, const char* who) {
    if (c->nz_n)
        return fail(c, DV_ERR_STATE, "%s: %lld noise rows are live, and a call without a landscape table senses without noise (dv_noise_clear first)",
                    who, (long long)c->nz_n);
    return DV_OK;
}

// The device's rows in the order of the call's landscape table (order: entry p is the caller's row order[p]; nullptr: the caller's order).
static int noise_upload(dv_ctx* c, const int* order) {
    if (!c->nz_n) return DV_OK;
    const size_t n = (size_t)c->nz_n;
    const NoiseRow* src = c->nz_rows.data();
    if (order) {
        c->nz_sorted.resize(n);
        for (size_t p = 0; p < n; ++p) c->nz_sorted[p] = c->nz_rows[(size_t)order[p]];
        src = c->nz_sorted.data();
    }
    return table_upload(c, c->nz_tab, src, n * sizeof(NoiseRow));
}

// lands_launch_sense's launch where rows are live (the rows uploaded by lands_upload, their count checked by lands_check).
static int noise_launch_sense(dv_ctx* c, long long p0, long long col0, int per, long long n, unsigned char* d_out, int* err) {
    const long long total = n * c->sensor.sh * c->sensor.sw;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (c->sn_tab)
        hipLaunchKernelGGL(k_sense_lands_sensors_noise, grid, dim3(256), 0, c->stream, c->ld_lands, c->ld_tab, c->sn_tab, c->sn_luts,
                           c->ld_of.device<int>(), c->nz_tab.device<NoiseRow>(), (unsigned)col0, (unsigned)per, c->d_poses + p0, (int)n, c->sensor, d_out,
                           err);
    else
        hipLaunchKernelGGL(k_sense_lands_noise, grid, dim3(256), 0, c->stream, c->ld_lands, c->ld_tab, c->ld_of.device<int>(),
                           c->nz_tab.device<NoiseRow>(), (unsigned)col0, (unsigned)per, c->d_poses + p0, (int)n, c->sensor, c->d_lut, d_out, err);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

extern "C" int dv_noise_rows(dv_ctx* c, uint64_t seed, const uint64_t* keys, const uint8_t* amp_s, const uint8_t* amp_v, int64_t n) {
    if (!c) return DV_ERR_INVALID;
    if (!keys || !amp_s || !amp_v) return fail(c, DV_ERR_INVALID, "dv_noise_rows: NULL argument");
    if (n < 1 || n > 0x7fffffff) return fail(c, DV_ERR_INVALID, "dv_noise_rows: n = %lld outside [1, 2^31)", (long long)n);
    if (!c->have_sensor) return fail(c, DV_ERR_STATE, "dv_noise_rows: sensor not configured (its w x h enters the rows' counters)");
    // The replacement first, in place only when it is complete.  Nothing goes to the device here: the next sensed call sends the rows
    // beside its landscape table, in that table's order (noise_upload), and not at all where the device holds the same already -- so
    // a step under fresh rows costs one copy, also where the call permutes them.
    std::vector<NoiseRow> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        rows[(size_t)i] = NoiseRow{dv::splitmix64(keys[i] + seed * 0x9E3779B97F4A7C15ull), amp_s[i], amp_v[i]};
    c->nz_rows.swap(rows);
    c->nz_keys.assign(keys, keys + n);
    c->nz_amp_s.assign(amp_s, amp_s + n);
    c->nz_amp_v.assign(amp_v, amp_v + n);
    c->nz_seed = seed;
    c->nz_n = n;
    return DV_OK;
}

extern "C" int dv_noise_clear(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    noise_drop(c);
    return DV_OK;
}

extern "C" int dv_noise_info(dv_ctx* c, int64_t* n, uint64_t* seed, uint64_t* keys, uint8_t* amp_s, uint8_t* amp_v) {
    if (!c) return DV_ERR_INVALID;
    if (n) *n = c->nz_n;
    if (seed) *seed = c->nz_seed;
    if (keys) std::copy(c->nz_keys.begin(), c->nz_keys.end(), keys);
    if (amp_s) std::copy(c->nz_amp_s.begin(), c->nz_amp_s.end(), amp_s);
    if (amp_v) std::copy(c->nz_amp_v.begin(), c->nz_amp_v.end(), amp_v);
    return DV_OK;
}
