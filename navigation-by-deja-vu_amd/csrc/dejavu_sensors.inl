// Sensor tables (include/dejavu.h: dv_sensors_*): a sensor configuration per landscape of the live landscape set.  Entry l is the sensor
// landscape l is sensed with: its pixel block SensorEntry { pw, ph, mask_n } and a level table uint8[3][256] of its own, the tables back
// to back in one allocation (entry l's at luts + 768 l).  The sensor's w x h stays the context's one (dv_configure_sensor): the
// one-value models and the route view store are built on it, and every sensing kernel finds a thread's pose as t / (sw sh).
//
// The table belongs to the entries of the set it was made for: dv_lands_set and dv_lands_clear drop it, as does a dv_configure_sensor
// that changes w x h (the masks were checked against that w).  With no table every call launches what it launched before there were
// tables: the forms below are kernels of their own, chosen by the host where a table is live.
//
//   k_sense_lands_sensors          k_sense_lands whose thread takes pw, ph, mask_n and the level table from its pose's entry as well.  A
//                                  wavefront may span poses of different entries when sw sh is no multiple of 64: their block loops
//                                  (pw ph trips) then differ in length, which is divergence and nothing more, since sense_thread has no
//                                  barrier.  The word per pose comes from the entry's own footprint (sw pw) x (sh ph).
//   k_mb_pose_bank_lands_sensors   (dejavu_mushroom.inl) k_mb_pose_bank_lands likewise; a workgroup is one column, so one entry.
//
// A pose with no landscape table (land_of_* == NULL) is on the context's landscape under the context's sensor, table or not.
namespace dv {

// land_of_column with the column's sensor: g's rows / cols and pw / ph / mask_n become the entry's, `lut` its level table.
__device__ __forceinline__ const unsigned char* land_sensor_of_column(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                                                      const SensorEntry* __restrict__ sens, const unsigned char* __restrict__ luts,
                                                                      const int* __restrict__ land_of, unsigned col, unsigned per, SensorCfg& g,
                                                                      const unsigned char*& lut) {
    const int l = land_of[col / per];
    const LandEntry e = tab[l];
    const SensorEntry s = sens[l];
    g.rows = e.rows;
    g.cols = e.cols;
    g.pw = s.pw;
    g.ph = s.ph;
    g.mask_n = s.mask_n;
    lut = luts + 768 * (size_t)l;
    return lands + e.base;
}

__global__ void k_sense_lands_sensors(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab, const SensorEntry* __restrict__ sens,
                                      const unsigned char* __restrict__ luts, const int* __restrict__ land_of, unsigned col0, unsigned per,
                                      const Pose* __restrict__ poses, int n, SensorCfg g, unsigned char* __restrict__ out, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pose = t / ((long long)g.sw * g.sh);
    if (pose >= n) return;                                     // (before the tables are read)
    const unsigned char* lut;
    const unsigned char* land = land_sensor_of_column(lands, tab, sens, luts, land_of, col0 + (unsigned)pose, per, g, lut);
    sense_thread<true>(land, poses, n, g, lut, out, err);
}

}  // namespace dv

static void sensors_free(dv_ctx* c) {
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->sn_tab); F(c->sn_luts);
    c->sn_pw.clear();
    c->sn_ph.clear();
    c->sn_mask.clear();
    c->sn_luts_host.clear();
}

// lands_launch_sense's launch where a sensor table is live.
static int sensors_launch_sense(dv_ctx* c, long long p0, long long col0, int per, long long n, unsigned char* d_out, int* err) {
    const long long total = n * c->sensor.sh * c->sensor.sw;
    hipLaunchKernelGGL(k_sense_lands_sensors, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->ld_lands, c->ld_tab, c->sn_tab,
                       c->sn_luts, c->ld_of.device<int>(), (unsigned)col0, (unsigned)per, c->d_poses + p0, (int)n, c->sensor, d_out, err);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

extern "C" int dv_sensors_set(dv_ctx* c, const int32_t* pw, const int32_t* ph, const int32_t* mask_n, const uint8_t* luts, int n) {
    if (!c) return DV_ERR_INVALID;
    if (!pw || !ph || !mask_n || !luts) return fail(c, DV_ERR_INVALID, "dv_sensors_set: NULL argument");
    if (!c->have_sensor) return fail(c, DV_ERR_STATE, "dv_sensors_set: sensor not configured (dv_configure_sensor sets the w x h all entries share)");
    int rc = lands_need(c, "dv_sensors_set");
    if (rc) return rc;
    const int L = (int)c->ld_rows.size();
    if (n != L) return fail(c, DV_ERR_INVALID, "dv_sensors_set: %d entries for a set of n_lands = %d landscapes", n, L);
    std::vector<SensorEntry> tab((size_t)n);
    for (int l = 0; l < n; ++l) {                                       // (what dv_configure_sensor asks of its own)
        if (pw[l] < 1 || ph[l] < 1 || (long long)pw[l] * ph[l] > 4096)
            return fail(c, DV_ERR_INVALID, "dv_sensors_set: entry %d: bad sensor pixel geometry %d x %d", l, (int)pw[l], (int)ph[l]);
        if (mask_n[l] < 0 || mask_n[l] > c->sensor.sw / 2)
            return fail(c, DV_ERR_INVALID, "dv_sensors_set: entry %d: mask_middle_n %d outside [0, %d]", l, (int)mask_n[l], c->sensor.sw / 2);
        tab[(size_t)l] = SensorEntry{pw[l], ph[l], mask_n[l]};
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // the replacement first, in place only when it is complete
    SensorEntry* t = nullptr;
    unsigned char* d = nullptr;
    const size_t lut_bytes = (size_t)n * 768;
    hipError_t e = hipMalloc((void**)&t, tab.size() * sizeof(SensorEntry));
    if (e == hipSuccess) e = hipMalloc((void**)&d, lut_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(t, tab.data(), tab.size() * sizeof(SensorEntry), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d, luts, lut_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // `tab` and `luts` are this call's; nothing reads the old table any more
    if (e != hipSuccess) {                                              // the old table stays as it was
        (void)hipGetLastError();
        if (t) (void)hipFree(t);
        if (d) (void)hipFree(d);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_sensors_set: %d entries: %s", n, hipGetErrorString(e));
    }
    if (c->sn_tab) (void)hipFree(c->sn_tab);
    if (c->sn_luts) (void)hipFree(c->sn_luts);
    c->sn_tab = t;
    c->sn_luts = d;
    c->sn_pw.assign(pw, pw + n);
    c->sn_ph.assign(ph, ph + n);
    c->sn_mask.assign(mask_n, mask_n + n);
    c->sn_luts_host.assign(luts, luts + lut_bytes);
    return DV_OK;
}

extern "C" int dv_sensors_clear(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    sensors_free(c);
    return DV_OK;
}

extern "C" int dv_sensors_info(dv_ctx* c, int* n, int32_t* pw, int32_t* ph, int32_t* mask_n, uint8_t* luts) {
    if (!c) return DV_ERR_INVALID;
    if (n) *n = (int)c->sn_pw.size();
    for (size_t l = 0; l < c->sn_pw.size(); ++l) {
        if (pw) pw[l] = c->sn_pw[l];
        if (ph) ph[l] = c->sn_ph[l];
        if (mask_n) mask_n[l] = c->sn_mask[l];
    }
    if (luts && !c->sn_luts_host.empty()) std::memcpy(luts, c->sn_luts_host.data(), c->sn_luts_host.size());
    return DV_OK;
}
