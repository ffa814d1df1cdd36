// Error / coverage metrics against SEVERAL routes (include/dejavu.h: dv_path_routes_*): update_error of the reference
// (navsim/NavBySceneFamiliarity.py:252-276) for the members of an ensemble whose trials were trained on routes of their own.  Included
// by dejavu_hip.hip; the kernel is k_path_error_routes (dejavu_kernels.h).  Nothing here touches the one-path calls' buffers
// (dv_set_training_path, dv_path_slots, ...), and those calls touch nothing here.
//
// The device never sees an index the host has not checked: the routes' bounds when they are set, every slot's route when the slots are
// made, every entry's slot before a call's first enqueue.  A call that is refused, or that cannot allocate, leaves routes, slots and marks
// as they were: what replaces them is made first, and put in their place only when all of it is there.

static void path_routes_free(dv_ctx* c) {
    if (c->rt_xy) { (void)hipFree(c->rt_xy); c->rt_xy = nullptr; }
    if (c->rt_cover) { (void)hipFree(c->rt_cover); c->rt_cover = nullptr; }
    if (c->rt_tab) { (void)hipFree(c->rt_tab); c->rt_tab = nullptr; }
    if (c->rt_tab_host) { (void)hipHostFree(c->rt_tab_host); c->rt_tab_host = nullptr; }
    c->rt_tab_cap = c->rt_tab_host_cap = 0;
    c->rt_first.clear();
    c->rt_slot_route.clear();
    c->rt_slot_first.clear();
}

static int path_routes_hip_error(dv_ctx* c, const char* who, hipError_t e) {
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
}

static int path_routes_need(dv_ctx* c, const char* who, bool slots) {
    if (c->rt_first.empty()) return fail(c, DV_ERR_STATE, "%s: no routes set (dv_path_routes_set)", who);
    if (slots && c->rt_slot_route.empty()) return fail(c, DV_ERR_STATE, "%s: no slots (dv_path_routes_slots)", who);
    return DV_OK;
}

extern "C" int dv_path_routes_set(dv_ctx* c, const double* xy, const int64_t* first, int n_routes) {
    if (!c) return DV_ERR_INVALID;
    if (n_routes < 0) return fail(c, DV_ERR_INVALID, "dv_path_routes_set: n_routes %d < 0", n_routes);
    const bool detach = !xy || !first || n_routes == 0;
    if (!detach) {
        if (first[0] != 0) return fail(c, DV_ERR_INVALID, "dv_path_routes_set: first[0] = %lld, not 0", (long long)first[0]);
        for (int r = 0; r < n_routes; ++r)
            if (first[r + 1] <= first[r])
                return fail(c, DV_ERR_INVALID, "dv_path_routes_set: first[%d] = %lld does not rise above first[%d] = %lld (a route has at least one point)",
                            r + 1, (long long)first[r + 1], r, (long long)first[r]);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double* pts = nullptr;
    if (!detach) {
        const size_t bytes = (size_t)first[n_routes] * 2 * sizeof(double);
        hipError_t e = hipMalloc((void**)&pts, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(pts, xy, bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);              // `xy` is borrowed for this call only
        if (e != hipSuccess) {
            if (pts) (void)hipFree(pts);
            return path_routes_hip_error(c, "dv_path_routes_set", e);
        }
    }
    // the routes the slots were made for are gone: so are the slots and their marks
    if (c->rt_xy) (void)hipFree(c->rt_xy);
    if (c->rt_cover) { (void)hipFree(c->rt_cover); c->rt_cover = nullptr; }
    c->rt_slot_route.clear();
    c->rt_slot_first.clear();
    c->rt_xy = pts;
    if (detach) c->rt_first.clear();
    else c->rt_first.assign(first, first + n_routes + 1);
    return DV_OK;
}

extern "C" int dv_path_routes_slots(dv_ctx* c, const int32_t* route_of_slot, int n_slots) {
    if (!c) return DV_ERR_INVALID;
    int rc = path_routes_need(c, "dv_path_routes_slots", false);
    if (rc) return rc;
    if (n_slots < 0) return fail(c, DV_ERR_INVALID, "dv_path_routes_slots: n_slots %d < 0", n_slots);
    if (n_slots > 0) rc = index_check(c, "dv_path_routes_slots", "route_of_slot", route_of_slot, n_slots, (int)c->rt_first.size() - 1, "n_routes");
    if (rc) return rc;
    std::vector<int64_t> base((size_t)n_slots + 1, 0);
    for (int j = 0; j < n_slots; ++j) {
        const int r = route_of_slot[j];
        base[(size_t)j + 1] = base[(size_t)j] + (c->rt_first[(size_t)r + 1] - c->rt_first[(size_t)r]);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned char* cover = nullptr;
    if (n_slots > 0) {
        const size_t bytes = (size_t)base[(size_t)n_slots];
        hipError_t e = hipMalloc((void**)&cover, bytes);
        if (e == hipSuccess) e = hipMemsetAsync(cover, 0, bytes, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            if (cover) (void)hipFree(cover);
            return path_routes_hip_error(c, "dv_path_routes_slots", e);
        }
    }
    if (c->rt_cover) (void)hipFree(c->rt_cover);
    c->rt_cover = cover;
    if (n_slots > 0) {
        c->rt_slot_route.assign(route_of_slot, route_of_slot + n_slots);
        c->rt_slot_first.swap(base);
    } else {
        c->rt_slot_route.clear();
        c->rt_slot_first.clear();
    }
    return DV_OK;
}

extern "C" int dv_path_routes_error(dv_ctx* c, const int32_t* slots, const double* x, const double* y, const double* reach, int64_t n,
                                    double* nearest) {
    if (!c) return DV_ERR_INVALID;
    int rc = path_routes_need(c, "dv_path_routes_error", true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!slots || !x || !y || !reach || !nearest)))
        return fail(c, DV_ERR_INVALID, "dv_path_routes_error: NULL argument or n < 0");
    if (n == 0) return DV_OK;
    rc = index_check(c, "dv_path_routes_error", "slots", slots, n, (int)c->rt_slot_route.size(), "n_slots");
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // the call's table: n entries, then n minima that start as all ones -- one upload for both
    const size_t tab_bytes = (size_t)n * sizeof(PathRouteEntry), bytes = tab_bytes + (size_t)n * sizeof(unsigned long long);
    if (bytes > c->rt_tab_host_cap) {
        unsigned char* h = nullptr;
        hipError_t e = hipHostMalloc((void**)&h, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return path_routes_hip_error(c, "dv_path_routes_error", e);
        if (c->rt_tab_host) (void)hipHostFree(c->rt_tab_host);       // (every call waits for its copies before it returns)
        c->rt_tab_host = h;
        c->rt_tab_host_cap = bytes;
    }
    rc = grow_buffer(c, c->rt_tab, c->rt_tab_cap, bytes);
    if (rc) return rc;
    PathRouteEntry* tab = reinterpret_cast<PathRouteEntry*>(c->rt_tab_host);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(c->rt_tab_host + tab_bytes);
    int64_t longest = 0;
    for (int64_t i = 0; i < n; ++i) {
        const size_t s = (size_t)slots[i], r = (size_t)c->rt_slot_route[s];
        PathRouteEntry& e = tab[i];
        e.first = (long long)c->rt_first[r];
        e.n = (long long)(c->rt_first[r + 1] - c->rt_first[r]);
        e.cover = (long long)c->rt_slot_first[s];
        e.x = x[i]; e.y = y[i]; e.reach = reach[i];
        keys[i] = ~0ull;
        if (e.n > longest) longest = e.n;
    }
    int64_t nb = (longest + kPathRoutePoints - 1) / kPathRoutePoints;
    if (nb > 256) nb = 256;
    HIP_TRY(c, hipMemcpyAsync(c->rt_tab, c->rt_tab_host, bytes, hipMemcpyHostToDevice, c->stream));
    unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(c->rt_tab + tab_bytes);
    constexpr int64_t kMaxGridY = 65535;
    for (int64_t j0 = 0; j0 < n; j0 += kMaxGridY) {
        const int64_t cnt = n - j0 < kMaxGridY ? n - j0 : kMaxGridY;
        hipLaunchKernelGGL(k_path_error_routes, dim3((unsigned)nb, (unsigned)cnt), dim3(256), 0, c->stream, (const double*)c->rt_xy, c->rt_cover,
                           (const PathRouteEntry*)c->rt_tab, d_keys, (long long)j0);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(keys, d_keys, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(nearest, keys, (size_t)n * sizeof(double));
    return DV_OK;
}

static int path_routes_slot(dv_ctx* c, const char* who, int slot) {
    const int n_slots = (int)c->rt_slot_route.size();
    if (slot < 0 || slot >= n_slots) return fail(c, DV_ERR_INVALID, "%s: slot %d outside [0, n_slots = %d)", who, slot, n_slots);
    return DV_OK;
}

extern "C" int dv_path_routes_coverage(dv_ctx* c, int slot, uint8_t* out, int64_t n) {
    if (!c) return DV_ERR_INVALID;
    int rc = path_routes_need(c, "dv_path_routes_coverage", true);
    if (rc) return rc;
    rc = path_routes_slot(c, "dv_path_routes_coverage", slot);
    if (rc) return rc;
    if (!out) return fail(c, DV_ERR_INVALID, "dv_path_routes_coverage: out is NULL");
    const int64_t at = c->rt_slot_first[(size_t)slot], len = c->rt_slot_first[(size_t)slot + 1] - at;
    if (n != len) return fail(c, DV_ERR_INVALID, "dv_path_routes_coverage: n = %lld, but slot %d's route has %lld points", (long long)n, slot, (long long)len);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->rt_cover + at, (size_t)len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DV_OK;
}

extern "C" int dv_path_routes_reset(dv_ctx* c, int slot) {
    if (!c) return DV_ERR_INVALID;
    int rc = path_routes_need(c, "dv_path_routes_reset", true);
    if (rc) return rc;
    int64_t at = 0, len = c->rt_slot_first.back();                // slot < 0: all of them
    if (slot >= 0) {
        rc = path_routes_slot(c, "dv_path_routes_reset", slot);
        if (rc) return rc;
        at = c->rt_slot_first[(size_t)slot];
        len = c->rt_slot_first[(size_t)slot + 1] - at;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->rt_cover + at, 0, (size_t)len, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DV_OK;
}

extern "C" int dv_path_routes_info(dv_ctx* c, int* n_routes, int* n_slots, int64_t* n_points) {
    if (!c) return DV_ERR_INVALID;
    if (n_routes) *n_routes = c->rt_first.empty() ? 0 : (int)c->rt_first.size() - 1;
    if (n_slots) *n_slots = (int)c->rt_slot_route.size();
    if (n_points) *n_points = c->rt_first.empty() ? 0 : c->rt_first.back();
    return DV_OK;
}
