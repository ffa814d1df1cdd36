// Landscape sets (include/dejavu.h: dv_lands_*): several HSV landscapes of any shapes resident together, and a landscape index per
// pose in the sensed calls of the banked models.  The set is one allocation, the landscapes back to back with no padding (a 211 x 173
// landscape is 109 509 bytes, so its successor begins at an odd byte: the sensor model reads bytes, sense_fetch, and asks for no
// alignment), and a table LandEntry { base, rows, cols }[n_lands] beside it.  The sensor geometry, the level table and the mask are
// the context's one configuration (dv_configure_sensor) unless the set has a sensor table (dejavu_sensors.inl), which gives every
// landscape a pixel block, a mask and a level table of its own; dv_set_landscape's landscape, d_land, and every call that reads it
// are untouched by a set, and the set by them.
//
// A pose's landscape is land_of[(col0 + pose) / per], the rule mb_bank uses for banks: per = 1 in training (a landscape per view),
// per = A in an ensemble's step (a landscape per member), col0 the launch's first column within the call.
//
//   k_sense_lands          k_sense_each with the pose's own landscape: the thread forms a SensorCfg whose rows / cols are the entry's
//                          and runs sense_thread<true> on lands + base.  The arithmetic, the wrap of a negative index (by the pose's
//                          own rows and cols) and the word per pose are sense_thread's.
//   k_mb_pose_bank_lands   (dejavu_mushroom.inl) k_mb_pose_bank whose mb_fill_pose reads the workgroup's member's landscape.
//
// The host checks every entry of a landscape table against [0, n_lands) before a call's first enqueue, and keeps what the device's
// table holds so that an unchanged one is not sent again (index_check and table_upload).
namespace dv {

// The landscape of column `col` of a call: g's rows / cols become the entry's; returns the landscape's first byte.
__device__ __forceinline__ const unsigned char* land_of_column(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                                               const int* __restrict__ land_of, unsigned col, unsigned per, SensorCfg& g) {
    const LandEntry e = tab[land_of[col / per]];
    g.rows = e.rows;
    g.cols = e.cols;
    return lands + e.base;
}

// poses, out and err begin at this launch's first pose, which is column col0 of the call; the landscape table is the whole call's.
__global__ void k_sense_lands(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab, const int* __restrict__ land_of,
                              unsigned col0, unsigned per, const Pose* __restrict__ poses, int n, SensorCfg g,
                              const unsigned char* __restrict__ lut, unsigned char* __restrict__ out, int* __restrict__ err) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pose = t / ((long long)g.sw * g.sh);
    if (pose >= n) return;                                     // (before the table is read: sense_thread's own test comes after)
    const unsigned char* land = land_of_column(lands, tab, land_of, col0 + (unsigned)pose, per, g);
    sense_thread<true>(land, poses, n, g, lut, out, err);
}

}  // namespace dv

static int sensors_launch_sense(dv_ctx* c, long long p0, long long col0, int per, long long n, unsigned char* d_out, int* err);   // (dejavu_sensors.inl)
static int noise_launch_sense(dv_ctx* c, long long p0, long long col0, int per, long long n, unsigned char* d_out, int* err);     // (dejavu_noise.inl)
static int noise_check(dv_ctx* c, const char* who, const char* what, int64_t n);
static int noise_upload(dv_ctx* c, const int* order);

static void lands_free(dv_ctx* c) {
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    sensors_free(c);                                           // (a sensor table belongs to the entries of its set)
    F(c->ld_lands); F(c->ld_tab); F(c->ld_err);
    c->ld_err_cap = 0;
    table_free(c->ld_of);
    c->ld_bytes = 0;
    c->ld_rows.clear();
    c->ld_cols.clear();
    c->ld_err_host.clear();
}

static int lands_need(dv_ctx* c, const char* who) {
    if (!c->ld_lands) return fail(c, DV_ERR_STATE, "%s: no landscape set (dv_lands_set first)", who);
    return DV_OK;
}

// A call's landscape table, checked entry by entry before anything of the call reaches the device ...
static int lands_check(dv_ctx* c, const char* who, const char* what, const int32_t* land_of, int64_t n) {
    if (land_of) { const int rc = lands_need(c, who); if (rc) return rc; }   // (a NULL table is refused first, whether there is a set or not)
    const int rc = index_check(c, who, what, land_of, n, (int)c->ld_rows.size(), "n_lands");
    return rc ? rc : noise_check(c, who, what, n);             // (live noise rows: one per entry of this table, dejavu_noise.inl)
}

// ... and then enqueued for the device, unless the device's table holds the same already (`land_of` may be a temporary of the caller's).
// Live noise rows ride along, in the order of the table's entries: `order` (nullptr: the caller's own) is the permutation a call has
// given its table, entry p being the caller's order[p].
static int lands_upload(dv_ctx* c, const int32_t* land_of, int64_t n, const int* order = nullptr) {
    const int rc = table_upload(c, c->ld_of, land_of, (size_t)n * sizeof(int));
    return rc ? rc : noise_upload(c, order);
}

// Enqueue k_sense_lands for `n` poses that are resident in d_poses from `p0` on and are columns col0 .. of the call, into d_out
// (uint8[n][sh][sw][3]); err: int[n], zeroed by the caller.  Where the set has a sensor table (dejavu_sensors.inl) the pose's sensor is
// its landscape's entry, through the kernel form that reads the table; where noise rows are live (dejavu_noise.inl), the noise forms.
static int lands_launch_sense(dv_ctx* c, long long p0, long long col0, int per, long long n, unsigned char* d_out, int* err) {
    if (c->nz_n) return noise_launch_sense(c, p0, col0, per, n, d_out, err);
    if (c->sn_tab) return sensors_launch_sense(c, p0, col0, per, n, d_out, err);
    const long long total = n * c->sensor.sh * c->sensor.sw;
    hipLaunchKernelGGL(k_sense_lands, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->ld_lands, c->ld_tab, c->ld_of.device<int>(),
                       (unsigned)col0, (unsigned)per, c->d_poses + p0, (int)n, c->sensor, c->d_lut, d_out, err);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// Sense n poses, pose v on landscape land_of[v] (checked and uploaded by the caller), into d_sense; a word per pose in ld_err.
static int lands_enqueue_sense(dv_ctx* c, const double* x, const double* y, const double* angle, long long n) {
    int rc = grow_buffer(c, c->ld_err, c->ld_err_cap, (size_t)n * sizeof(int));
    if (!rc) rc = upload_member_poses(c, x, y, angle, (int)n, 1);   // (n members of one heading each: pose v is (x[v], y[v], angle[v]))
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->ld_err, 0, (size_t)n * sizeof(int), c->stream));
    return lands_launch_sense(c, 0, 0, 1, n, c->d_sense, c->ld_err);
}

// Wait for the stream and read the words: DV_ERR_INDEX names the first pose whose footprint left its own landscape.
static int lands_check_sense_error(dv_ctx* c, const char* who, long long n) {
    c->ld_err_host.resize((size_t)n);
    HIP_TRY(c, hipMemcpyAsync(c->ld_err_host.data(), c->ld_err, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (long long v = 0; v < n; ++v)
        if (c->ld_err_host[(size_t)v]) {
            const int l = c->ld_of.record<int>()[(size_t)v];
            return fail(c, DV_ERR_INDEX, "%s: the sensor footprint of pose %lld reaches past the end of its landscape %d (%d x %d) (index out of bounds)",
                        who, v, l, c->ld_rows[(size_t)l], c->ld_cols[(size_t)l]);
        }
    return DV_OK;
}

extern "C" int dv_lands_set(dv_ctx* c, const uint8_t* lands, const int32_t* rows, const int32_t* cols, int n_lands, int channels) {
    if (!c) return DV_ERR_INVALID;
    if (!lands || !rows || !cols) return fail(c, DV_ERR_INVALID, "dv_lands_set: NULL argument");
    if (n_lands < 1) return fail(c, DV_ERR_INVALID, "dv_lands_set: n_lands %d < 1", n_lands);
    if (channels != 3) return fail(c, DV_ERR_INVALID, "dv_lands_set: the landscapes must be uint8[rows, cols, 3]");
    std::vector<LandEntry> tab((size_t)n_lands);
    long long bytes = 0;
    for (int l = 0; l < n_lands; ++l) {
        if (rows[l] < 1 || cols[l] < 1) return fail(c, DV_ERR_INVALID, "dv_lands_set: landscape %d is %d x %d", l, (int)rows[l], (int)cols[l]);
        tab[(size_t)l] = LandEntry{bytes, rows[l], cols[l]};
        bytes += (long long)rows[l] * cols[l] * 3;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // the replacement first, in place only when it is complete
    unsigned char* d = nullptr;
    LandEntry* t = nullptr;
    hipError_t e = hipMalloc((void**)&d, (size_t)bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&t, tab.size() * sizeof(LandEntry));
    if (e == hipSuccess) e = hipMemcpyAsync(d, lands, (size_t)bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t, tab.data(), tab.size() * sizeof(LandEntry), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // `lands` and `tab` are this call's; nothing reads the old set any more
    if (e != hipSuccess) {                                              // the old set stays as it was
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        if (t) (void)hipFree(t);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_lands_set: %d landscapes of %lld bytes: %s", n_lands, bytes,
                    hipGetErrorString(e));
    }
    if (c->ld_lands) (void)hipFree(c->ld_lands);
    if (c->ld_tab) (void)hipFree(c->ld_tab);
    c->ld_lands = d;
    c->ld_tab = t;
    c->ld_bytes = bytes;
    c->ld_rows.assign(rows, rows + n_lands);
    c->ld_cols.assign(cols, cols + n_lands);
    sensors_free(c);                                                    // (the entries a sensor table belonged to are gone)
    return DV_OK;
}

extern "C" int dv_lands_clear(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    lands_free(c);
    return DV_OK;
}

extern "C" int dv_lands_info(dv_ctx* c, int* n_lands, int32_t* rows, int32_t* cols, int64_t* bytes) {
    if (!c) return DV_ERR_INVALID;
    if (n_lands) *n_lands = (int)c->ld_rows.size();
    for (size_t l = 0; l < c->ld_rows.size(); ++l) {
        if (rows) rows[l] = c->ld_rows[l];
        if (cols) cols[l] = c->ld_cols[l];
    }
    if (bytes) *bytes = (int64_t)c->ld_bytes;
    return DV_OK;
}

extern "C" int dv_lands_sense(dv_ctx* c, const double* x, const double* y, const double* angle, const int32_t* land_of_pose, int n, uint8_t* out) {
    if (!c) return DV_ERR_INVALID;
    if (!x || !y || !angle || !out || n < 1) return fail(c, DV_ERR_INVALID, "dv_lands_sense: NULL argument or n < 1");
    if (!c->have_sensor) return fail(c, DV_ERR_STATE, "sensor not configured");
    int rc = lands_check(c, "dv_lands_sense", "land_of_pose", land_of_pose, n);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * c->sensor.sh * c->sensor.sw * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (!rc) rc = lands_upload(c, land_of_pose, n);
    if (!rc) rc = lands_enqueue_sense(c, x, y, angle, n);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, c->d_sense, bytes, hipMemcpyDeviceToHost, c->stream));
    return lands_check_sense_error(c, "dv_lands_sense", n);
}
