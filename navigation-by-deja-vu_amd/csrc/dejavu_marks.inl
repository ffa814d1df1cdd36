// The three coverage statistics of a trial's result row, taken from the coverage marks where they lie (include/dejavu.h: dv_marks_*):
// percent_recapitulated, percent_recapitulated_forgiving and n_captures of the reference (navsim/NavBySceneFamiliarity.py:212-249).
// Included by dejavu_hip.hip after dejavu_path_routes.inl, whose table buffers (rt_tab, rt_tab_host) the calls here share: every call
// of either file waits for its copies before it returns, so the buffers are never in use by two calls.
//
// All three are functions of run[p], the number of consecutive set marks ending at p inclusive (0 where mark p is clear).  With n marks
// and a window of win marks:
//     covered  = #{p : marks[p] != 0}
//     furthest = max{p + 1 : run[p] >= win}, 0 when there is none        (the forgiving coverage is furthest / n)
//     captures = #{p in [win, n) : run[p] == win}                       (a run of win marks with a clear mark before it)
// The reference's loops ask np.all over a window per point.  The forgiving loop's "the win marks before i are all set" is
// run[i - 1] >= win.  The capture loop's "mark i is clear and the win marks after it are set" is a run that ends at p = i + win and is
// exactly win long; i >= 0 makes p >= win.  win == 0 (furthest = n, captures = the clear marks) and win > n (both 0) need no case of
// their own.
//
// k_marks_summary: one workgroup of 256 threads per entry { at, n, win } of a table, over a base pointer of marks.  A trip takes
// DV_MARKS_PER_TRIP marks, DV_MARKS_PER_THREAD consecutive ones per thread, read as BYTES -- a slot's marks begin at any byte (routes of
// odd length lie back to back in rt_cover) -- and kept as a bit mask in a register, so memory is read once.  The thread's chunk reduces
// to (all set?, trailing run); the pairs are scanned (reset where a chunk is not all set) by shuffles within the wave and through LDS
// across the four waves, which gives every thread the run that enters its chunk; the run that leaves the last thread is carried into
// the next trip.  Each thread then walks its mask with that run and counts.  Sums and the maximum go through the wave, the four waves,
// and plain stores by thread 0.  The kernel only reads marks; no atomics, no inline assembly.
// Runs, indices and counts are 64-bit throughout: a route may be as long as an allocation allows.  Within a trip a run fits an int
// (it is at most DV_MARKS_PER_TRIP); the carry between trips does not, and is a long long.
//
// The device never sees an index the host has not checked: every slot against its range and every window against >= 0 before a call's
// first enqueue; a refused call enqueues nothing.
namespace dv {

constexpr int kMarksPerThread = DV_MARKS_PER_THREAD;
constexpr int kMarksPerTrip = DV_MARKS_PER_TRIP;
static_assert(kMarksPerTrip == 256 * kMarksPerThread && kMarksPerThread <= 32, "a trip is 256 threads' chunks; a chunk is one mask");

struct MarksEntry { long long at, n, win; };

// The chunk of kMarksPerThread marks at marks[start ..], of which those below n exist: bit k = mark start + k is set.
__device__ __forceinline__ unsigned marks_chunk(const unsigned char* __restrict__ marks, long long start, long long n) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < kMarksPerThread; ++k)
        if (start + k < n) m |= (marks[start + k] != 0 ? 1u : 0u) << k;
    return m;
}

// (all set, trailing run) of a stretch as one int: 2 run + all.  Left stretch a, then right stretch b.
__device__ __forceinline__ int marks_join(int a, int b) { return (b & 1) ? ((a & 1) | (((a >> 1) + (b >> 1)) << 1)) : b; }

__global__ void __launch_bounds__(256)
k_marks_summary(const unsigned char* __restrict__ base, const MarksEntry* __restrict__ tab, long long* __restrict__ out, long long j0) {
    __shared__ int wave_pair[2][4];
    __shared__ long long part[3][4];
    const long long j = j0 + blockIdx.x;
    const MarksEntry e = tab[j];
    const unsigned char* __restrict__ marks = base + e.at;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr unsigned kFull = kMarksPerThread == 32 ? ~0u : (1u << kMarksPerThread) - 1u;
    long long covered = 0, furthest = 0, captures = 0;
    long long carry = 0;                                          // the run that ends at the last mark of the trip before
    unsigned m = marks_chunk(marks, (long long)tid * kMarksPerThread, e.n);
    int trip = 0;
    for (long long t0 = 0; t0 < e.n; t0 += kMarksPerTrip, ++trip) {
        const long long start = t0 + (long long)tid * kMarksPerThread;
        // the next trip's marks are asked for before this trip's are worked on
        const unsigned m_next = t0 + kMarksPerTrip < e.n ? marks_chunk(marks, start + kMarksPerTrip, e.n) : 0u;
        // the chunk as a pair: all set -> its run is its length; else the set marks at its top (a chunk past n has none: m = 0)
        const int all = m == kFull;
        const int trail = all ? kMarksPerThread : __clz((int)(~(m << (32 - kMarksPerThread))));
        int incl = trail << 1 | all;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int left = __shfl_up(incl, o);
            if (lane >= o) incl = marks_join(left, incl);
        }
        if (lane == 63) wave_pair[trip & 1][wave] = incl;
        int before = __shfl_up(incl, 1);                         // the lanes before this one; none before lane 0
        if (lane == 0) before = 1;
        __syncthreads();                                          // (the next trip's pairs go to the other half: one barrier a trip)
        int head = 1, whole = 1;                                  // the waves before this thread's own; all four
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int p = wave_pair[trip & 1][w];
            if (w < wave) head = marks_join(head, p);
            whole = marks_join(whole, p);
        }
        before = marks_join(head, before);
        long long run = (long long)(before >> 1) + ((before & 1) ? carry : 0);
        carry = (long long)(whole >> 1) + ((whole & 1) ? carry : 0);
#pragma unroll
        for (int k = 0; k < kMarksPerThread; ++k) {
            const long long p = start + k;
            if (p < e.n) {
                const bool set = (m >> k) & 1u;
                run = set ? run + 1 : 0;
                covered += set ? 1 : 0;
                if (run >= e.win) furthest = p + 1;               // p rises: the last one is the maximum
                if (p >= e.win && run == e.win) ++captures;
            }
        }
        m = m_next;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        covered += __shfl_xor(covered, o);
        captures += __shfl_xor(captures, o);
        const long long other = __shfl_xor(furthest, o);
        furthest = other > furthest ? other : furthest;
    }
    if (lane == 0) { part[0][wave] = covered; part[1][wave] = furthest; part[2][wave] = captures; }
    __syncthreads();
    if (tid == 0) {
        long long c = 0, f = 0, k = 0;
        for (int w = 0; w < 4; ++w) {
            c += part[0][w];
            f = part[1][w] > f ? part[1][w] : f;
            k += part[2][w];
        }
        out[3 * j] = c;
        out[3 * j + 1] = f;
        out[3 * j + 2] = k;
    }
}

}  // namespace dv

// A call's table and results: n entries, then n x 3 results, in the pinned and the device buffer of dv_path_routes_error (grow-only;
// what replaces a buffer is made before the old one goes).
static int marks_reserve(dv_ctx* c, const char* who, size_t bytes) {
    if (bytes > c->rt_tab_host_cap) {
        unsigned char* h = nullptr;
        hipError_t e = hipHostMalloc((void**)&h, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return path_routes_hip_error(c, who, e);
        if (c->rt_tab_host) (void)hipHostFree(c->rt_tab_host);       // (every call waits for its copies before it returns)
        c->rt_tab_host = h;
        c->rt_tab_host_cap = bytes;
    }
    return grow_buffer(c, c->rt_tab, c->rt_tab_cap, bytes);
}

static int marks_windows(dv_ctx* c, const char* who, const int64_t* window, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (window[i] < 0) return fail(c, DV_ERR_INVALID, "%s: window[%lld] = %lld < 0", who, (long long)i, (long long)window[i]);
    return DV_OK;
}

// The entries lie in the pinned table (marks_reserve, then filled by the caller): one upload, a launch per 65 535 entries on the
// context's stream, one copy back, one wait.
static int marks_run(dv_ctx* c, const unsigned char* base, int64_t n, int64_t* out) {
    const size_t tab_bytes = (size_t)n * sizeof(MarksEntry), out_bytes = (size_t)n * 3 * sizeof(long long);
    long long* d_out = reinterpret_cast<long long*>(c->rt_tab + tab_bytes);
    HIP_TRY(c, hipMemcpyAsync(c->rt_tab, c->rt_tab_host, tab_bytes, hipMemcpyHostToDevice, c->stream));
    constexpr int64_t kMaxGrid = 65535;
    for (int64_t j0 = 0; j0 < n; j0 += kMaxGrid) {
        const int64_t cnt = n - j0 < kMaxGrid ? n - j0 : kMaxGrid;
        hipLaunchKernelGGL(k_marks_summary, dim3((unsigned)cnt), dim3(256), 0, c->stream, base, (const MarksEntry*)c->rt_tab, d_out, (long long)j0);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(c->rt_tab_host + tab_bytes, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(out, c->rt_tab_host + tab_bytes, out_bytes);
    return DV_OK;
}

extern "C" int dv_marks_summary(dv_ctx* c, int64_t window, int64_t* out3) {
    if (!c) return DV_ERR_INVALID;
    if (c->n_path < 1) return fail(c, DV_ERR_STATE, "dv_marks_summary: no training path set (dv_set_training_path)");
    if (!out3) return fail(c, DV_ERR_INVALID, "dv_marks_summary: out3 is NULL");
    if (window < 0) return fail(c, DV_ERR_INVALID, "dv_marks_summary: window = %lld < 0", (long long)window);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = marks_reserve(c, "dv_marks_summary", sizeof(MarksEntry) + 3 * sizeof(long long));
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->aux_stream));                  // the metrics enqueued beside the steps (dv_path_error_enqueue)
    *reinterpret_cast<MarksEntry*>(c->rt_tab_host) = MarksEntry{0, (long long)c->n_path, (long long)window};
    return marks_run(c, c->d_cover, 1, out3);
}

extern "C" int dv_marks_summary_slots(dv_ctx* c, const int32_t* slots, const int64_t* window, int n, int64_t* out) {
    if (!c) return DV_ERR_INVALID;
    if (c->n_path < 1 || c->n_cover_slots < 1)
        return fail(c, DV_ERR_STATE, "dv_marks_summary_slots: no coverage slots (dv_set_training_path, dv_path_slots)");
    if (n < 0 || (n > 0 && (!slots || !window || !out))) return fail(c, DV_ERR_INVALID, "dv_marks_summary_slots: NULL argument or n < 0");
    if (n == 0) return DV_OK;
    int rc = index_check(c, "dv_marks_summary_slots", "slots", slots, n, c->n_cover_slots, "n_slots");
    if (!rc) rc = marks_windows(c, "dv_marks_summary_slots", window, n);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = marks_reserve(c, "dv_marks_summary_slots", (size_t)n * (sizeof(MarksEntry) + 3 * sizeof(long long)));
    if (rc) return rc;
    MarksEntry* tab = reinterpret_cast<MarksEntry*>(c->rt_tab_host);
    for (int i = 0; i < n; ++i) tab[i] = MarksEntry{(long long)slots[i] * (long long)c->n_path, (long long)c->n_path, (long long)window[i]};
    return marks_run(c, c->d_cover_slots, n, out);
}

extern "C" int dv_marks_summary_routes(dv_ctx* c, const int32_t* slots, const int64_t* window, int64_t n, int64_t* out) {
    if (!c) return DV_ERR_INVALID;
    int rc = path_routes_need(c, "dv_marks_summary_routes", true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!slots || !window || !out))) return fail(c, DV_ERR_INVALID, "dv_marks_summary_routes: NULL argument or n < 0");
    if (n == 0) return DV_OK;
    rc = index_check(c, "dv_marks_summary_routes", "slots", slots, n, (int)c->rt_slot_route.size(), "n_slots");
    if (!rc) rc = marks_windows(c, "dv_marks_summary_routes", window, n);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = marks_reserve(c, "dv_marks_summary_routes", (size_t)n * (sizeof(MarksEntry) + 3 * sizeof(long long)));
    if (rc) return rc;
    MarksEntry* tab = reinterpret_cast<MarksEntry*>(c->rt_tab_host);
    for (int64_t i = 0; i < n; ++i) {
        const size_t s = (size_t)slots[i];
        tab[i] = MarksEntry{(long long)c->rt_slot_first[s], (long long)(c->rt_slot_first[s + 1] - c->rt_slot_first[s]), (long long)window[i]};
    }
    return marks_run(c, c->rt_cover, n, out);
}
