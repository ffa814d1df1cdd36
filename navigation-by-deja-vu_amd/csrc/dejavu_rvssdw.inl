// Windowed SSD on the route view store (include/dejavu.h: dv_rvssdw_*): dv_rvssd_*'s exact SSD with a temporal window.  Member i is
// scored against views [win_lo[i], win_hi[i]) of ITS OWN route only, at most DV_RVWIN_MAX_VIEWS of them.  The store, the view norms
// (k_rvssd_norms, kept per store and channel), the operand rows (k_rvssd_prep), the arithmetic of a view group (rvssd_group_acc,
// rvssd_value, rvssd_key_min) and the deciding launch (k_rvssd_best) are dejavu_rvssd.inl's; the window rule and the member's window
// (rvwin_check, RvWin) are dejavu_rvwin.inl's; the plan of a re-localising call (rvreloc_plan, the host's order tables) is
// dejavu_rvreloc.inl's.  A windowed step is sense -> prep -> k_rvssdw_score -> best.
//
//   k_rvssdw_score  workgroup = (a tile of at most kRvssdTile headings, one member), in the CALLER's column order: windows differ per
//                   member, so there is no route sort.  The window is not aligned to the store's groups of 64 views: the workgroup covers
//                   groups lo >> 6 .. (hi - 1) >> 6 (at most 9 for 512 views), wave w takes groups w, w + 4, w + 8.  A view outside
//                   [lo, hi) -- the rest of the first and last group, the route's padding views among them -- gets the key of all ones.
//                   Every wave keeps a running minimum per accumulator register over its groups; the four waves' minima meet in LDS
//                   behind one barrier, and threads 0 .. nc - 1 write ssd and view of their column straight into the caller's order.
//                   No atomics, no keys to clear, no unsort.
// With a threshold per member (reloc_below), between that launch and k_rvssd_best, in the same enqueue:
//   k_rvssdw_plan   ONE workgroup: rvreloc_plan with the sign of the scores turned (the familiarity is -SSD) and tiles of kRvssdTile
//                   columns: lost[], the lost columns' col_of, their tiles and the counts, by prefix sums.
//   k_rvssdw_whole  k_rvssd_score<0>'s body (rvssd_score_tile) on the device's plan, the operand rows read in the caller's order; the grid
//                   is sized on the host for "every member lost", a workgroup past the device's tile count returns at once.
//   k_rvssdw_unsort the lost columns' keys over the windowed ssd and view.
// k_rvssd_best then sets DV_RES_RELOCALISED from lost[].
namespace dv {

constexpr int kRvssdwMembersPerLaunch = 32768;   // members of a windowed scoring launch at most (a grid's y)
constexpr int kRvssdwAhead = 4;                  // K-steps of a view group whose loads are issued together (rvssd_group_acc)

// grid = (ceil(A / kRvssdTile), members of the launch), member i = i0 + blockIdx.y; op, pnorm: the caller's columns (k_rvssd_prep
// without a column table).
__global__ void __launch_bounds__(256)
k_rvssdw_score(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvWin* __restrict__ wins,
               const unsigned* __restrict__ op, const unsigned* __restrict__ pnorm, const unsigned* __restrict__ vnorm, int channel, int i0, int A,
               int Pw, int Kp, double* __restrict__ out_ssd, long long* __restrict__ out_view) {
    __shared__ unsigned long long mins[4][kRvssdTile];
    const int i = i0 + (int)blockIdx.y, c0 = (int)blockIdx.x * kRvssdTile;
    const int nc = A - c0 < kRvssdTile ? A - c0 : kRvssdTile;
    const RvWin win = wins[i];
    const RvRoute rt = routes[win.route];
    const int lo = win.lo, wend = win.hi;                                            // (0 <= lo < wend <= rt.len: checked on the host)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, hi = lane >> 5;
    const bool has_col = col < nc;
    const long long oc0 = (long long)i * A + c0;                                     // the tile's first column, in the caller's order
    const uint4* __restrict__ arow = reinterpret_cast<const uint4*>(op + (oc0 + (has_col ? col : 0)) * Kp * 8) + hi;
    // register r of a lane is (column m = (r & 3) + 8 (r >> 2) + 4 hi, view = lane & 31) of its half (k_rvssd_score's map)
    int pn[16];
    unsigned long long best[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * hi;
        pn[r] = (int)pnorm[oc0 + (m < nc ? m : 0)];
        best[r] = ~0ull;
    }
    const int g_last = (wend - 1) >> 6;
    for (int gl = (lo >> 6) + wave; gl <= g_last; gl += kRvssdGroupsPerBlock) {      // the wave's view groups within the route
        const unsigned* __restrict__ vb = planes + ((rt.g0 + gl) * 3 + channel) * Pw * 64 + col;
        v16i_t acc0, acc1;
        rvssd_group_acc<kRvssdwAhead>(arow, has_col, vb, hi, Pw, Kp, acc0, acc1);
        const long long f0 = (long long)gl * 64 + col, f1 = f0 + 32;               // the lane's two views within the route
        const bool live0 = f0 >= lo && f0 < wend, live1 = f1 >= lo && f1 < wend;
        const unsigned* __restrict__ vn = vnorm + (rt.g0 + gl) * 64 + col;
        const int vn0 = (int)vn[0], vn1 = (int)vn[32];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned long long key = rvssd_key_min(rvssd_value(vn0, pn[r], acc0[r]), rvssd_value(vn1, pn[r], acc1[r]), f0, f1, live0, live1);
            best[r] = key < best[r] ? key : best[r];
        }
    }
    if (col == 0) {                                                                  // (every lane of a half-wave holds its minima)
#pragma unroll
        for (int r = 0; r < 16; ++r) mins[wave][(r & 3) + 8 * (r >> 2) + 4 * hi] = best[r];
    }
    __syncthreads();
    if ((int)threadIdx.x < nc) {
        const int m = (int)threadIdx.x;
        unsigned long long key = mins[0][m];
#pragma unroll
        for (int w = 1; w < 4; ++w) key = mins[w][m] < key ? mins[w][m] : key;
        out_ssd[oc0 + m] = (double)(unsigned)(key >> 32);
        out_view[oc0 + m] = (long long)(key & 0xffffffffull);
    }
}

// rvreloc_plan on SSDs: fam = -ssd.  One workgroup.
__global__ void __launch_bounds__(256)
k_rvssdw_plan(const double* __restrict__ ssd, const int* __restrict__ err, const double* __restrict__ tau, const int* __restrict__ route_of,
              const int* __restrict__ order, const int* __restrict__ run0, const int* __restrict__ run1, int n, int A, int* __restrict__ lost,
              int* pm, int* col_of, RvTile* __restrict__ tiles, int* __restrict__ cnt) {
    __shared__ int ws[4];
    rvreloc_plan<1>(ssd, err, tau, route_of, order, run0, run1, n, A, kRvssdTile, lost, pm, col_of, tiles, cnt, ws);
}

// k_rvssd_score<0> on the device's plan: tile t0 + blockIdx.y of cnt[0]; keys[s] of the plan's column s; the operand rows and norms
// are the caller's columns' (col_of[s]).  grid = (ceil(groups of the longest route / 4), tiles of the launch).
__global__ void __launch_bounds__(256)
k_rvssdw_whole(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvTile* __restrict__ tiles,
               const int* __restrict__ col_of, const unsigned* __restrict__ op, const unsigned* __restrict__ pnorm,
               const unsigned* __restrict__ vnorm, int channel, int A, int P, int Pw, int Kp, unsigned long long* __restrict__ keys, int t0,
               const int* __restrict__ cnt) {
    const int t = t0 + (int)blockIdx.y;
    if (t >= cnt[0]) return;                                                         // (the whole workgroup)
    rvssd_score_tile<0, 1>(planes, routes, tiles[t], (int)blockIdx.x, col_of, op, pnorm, vnorm, channel, A, P, Pw, Kp, keys, nullptr, nullptr);
}

// keys[s] of the plan's cnt[1] columns -> ssd[col_of[s]], view[col_of[s]], over the windowed ones; grid = ceil(C / 256).
__global__ void __launch_bounds__(256)
k_rvssdw_unsort(const unsigned long long* __restrict__ keys, const int* __restrict__ col_of, const int* __restrict__ cnt, double* __restrict__ ssd,
                long long* __restrict__ view) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= cnt[1]) return;
    const unsigned long long key = keys[s];
    ssd[col_of[s]] = (double)(unsigned)(key >> 32);
    view[col_of[s]] = (long long)(key & 0xffffffffull);
}

}  // namespace dv

// dv_rvssd_*'s checks, dv_rvwin_*'s window rule and (with thresholds) dv_rvreloc_*'s, before anything of the call reaches the device.
static int rvssdw_check(dv_ctx* c, const char* who, int N, int A, const int32_t* route_of_member, const int32_t* win_lo, const int32_t* win_hi,
                        const double* reloc_below, int channel) {
    int rc = rvssd_check_tables(c, who, N, A, route_of_member, channel);
    if (rc) return rc;
    const std::vector<double> no_weights((size_t)N, 0.0);                            // (SSD has no chemical weight)
    rc = rvwin_check(c, who, N, A, route_of_member, no_weights.data(), win_lo, win_hi);
    if (!rc && reloc_below) rc = rvreloc_check(c, who, N, A, reloc_below);
    return rc;
}

// Score the N * A columns whose patches lie in d_sense, member i against its window; err: a word per column, or nullptr.  The call's
// tables travel in one copy to a table of their own (rvsw_tab).  reloc_below (or nullptr): the members' thresholds; the tables grow by
// the route-sorted order of ALL members (one group: SSD has no score buffer to fit) and the chain by the plan, the whole-route scoring
// of the lost columns and their write-back, between the windowed scoring and the deciding launch.
static int rvssdw_run(dv_ctx* c, int N, int A, const int32_t* route_of_member, const int32_t* win_lo, const int32_t* win_hi,
                      const double* reloc_below, int channel, const int* err, double* angle_ssd, int64_t* angle_view, int32_t* best_heading,
                      uint32_t* member_flags) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4, Kp = (P + 31) / 32, C = N * A;
    std::vector<unsigned char> tab((size_t)N * sizeof(RvWin), 0);
    RvWin* win = reinterpret_cast<RvWin*>(tab.data());
    for (int i = 0; i < N; ++i) win[i] = RvWin{route_of_member[i], win_lo[i], win_hi[i], 0};
    RvReloc reloc;
    if (reloc_below) {
        reloc.N = N; reloc.A = A; reloc.T = kRvssdTile; reloc.gm = N; reloc.lstride = 0;
        rvreloc_order_tables(reloc, route_of_member, reloc_below, tab);
    }
    int rc = table_upload(c, c->rvsw_tab, tab.data(), tab.size());
    if (!rc && reloc_below) rc = grow_buffer(c, c->rvs_plan, c->rvs_plan_cap, rvreloc_plan_bytes(reloc));
    if (!rc && reloc_below) rc = grow_buffer(c, c->rvs_keys, c->rvs_keys_cap, (size_t)C * sizeof(unsigned long long));
    const size_t out_bytes = (size_t)C * 16 + (size_t)N * 8;
    if (!rc) rc = grow_buffer(c, c->rvs_out, c->rvs_out_cap, out_bytes);
    unsigned* vnorm = nullptr;
    if (!rc) rc = rvssd_norms_and_rows(c, channel, C, vnorm);
    if (rc) return rc;
    unsigned* pnorm = c->rvs_op + (size_t)C * Kp * 8;
    const RvWin* wins = reinterpret_cast<const RvWin*>(c->rvsw_tab.dev);
    double* d_ssd = reinterpret_cast<double*>(c->rvs_out);
    long long* d_view = reinterpret_cast<long long*>(c->rvs_out + (size_t)C * 8);
    int* d_best = reinterpret_cast<int*>(c->rvs_out + (size_t)C * 16);
    unsigned* d_flags = reinterpret_cast<unsigned*>(c->rvs_out + (size_t)C * 16 + (size_t)N * 4);
    hipLaunchKernelGGL(k_rvssd_prep, dim3((unsigned)C), dim3(256), 0, c->stream, c->d_sense, (const int*)nullptr, channel, P, Kp, c->rvs_op, pnorm);
    const unsigned tiles_x = (unsigned)((A + kRvssdTile - 1) / kRvssdTile);
    for (int i0 = 0; i0 < N; i0 += kRvssdwMembersPerLaunch) {                        // (members are a grid's y)
        const unsigned ni = (unsigned)std::min(N - i0, kRvssdwMembersPerLaunch);
        hipLaunchKernelGGL(k_rvssdw_score, dim3(tiles_x, ni), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, wins, c->rvs_op, pnorm, vnorm,
                           channel, i0, A, Pw, Kp, d_ssd, d_view);
    }
    HIP_TRY(c, hipGetLastError());
    const int* lost = nullptr;
    if (reloc_below) {
        const RvRelocDev d = rvreloc_dev(c->rvs_plan, reloc);
        const unsigned char* t = c->rvsw_tab.dev;
        hipLaunchKernelGGL(k_rvssdw_plan, dim3(1), dim3(256), 0, c->stream, d_ssd, err, reinterpret_cast<const double*>(t + reloc.off_tau),
                           reinterpret_cast<const int*>(t + reloc.off_route), reinterpret_cast<const int*>(t + reloc.off_order),
                           reinterpret_cast<const int*>(t + reloc.off_run0), reinterpret_cast<const int*>(t + reloc.off_run1), N, A, d.lost, d.pm,
                           d.col_of, d.tiles, d.cnt);
        HIP_TRY(c, hipMemsetAsync(c->rvs_keys, 0xff, (size_t)C * sizeof(unsigned long long), c->stream));
        const unsigned gchunks = (unsigned)(((c->rv_lmax + 63) / 64 + kRvssdGroupsPerBlock - 1) / kRvssdGroupsPerBlock);
        for (int t0 = 0; t0 < reloc.max_tiles; t0 += kRvssdTilesPerLaunch) {         // (sized for "every member lost")
            const int nt = std::min(reloc.max_tiles - t0, kRvssdTilesPerLaunch);
            hipLaunchKernelGGL(k_rvssdw_whole, dim3(gchunks, (unsigned)nt), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, d.tiles, d.col_of,
                               c->rvs_op, pnorm, vnorm, channel, A, P, Pw, Kp, c->rvs_keys, t0, d.cnt);
        }
        hipLaunchKernelGGL(k_rvssdw_unsort, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, c->stream, c->rvs_keys, d.col_of, d.cnt, d_ssd, d_view);
        HIP_TRY(c, hipGetLastError());
        lost = d.lost;
    }
    hipLaunchKernelGGL(k_rvssd_best, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, d_ssd, err, lost, N, A, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    c->rv_out_host.resize(out_bytes);
    HIP_TRY(c, hipMemcpyAsync(c->rv_out_host.data(), c->rvs_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned char* h = c->rv_out_host.data();
    std::memcpy(angle_ssd, h, (size_t)C * 8);
    if (angle_view) std::memcpy(angle_view, h + (size_t)C * 8, (size_t)C * 8);
    std::memcpy(best_heading, h + (size_t)C * 16, (size_t)N * 4);
    if (member_flags) std::memcpy(member_flags, h + (size_t)C * 16 + (size_t)N * 4, (size_t)N * 4);
    return DV_OK;
}

extern "C" int dv_rvssdw_step_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member,
                                 const int32_t* win_lo, const int32_t* win_hi, const double* reloc_below, int channel, double* angle_ssd,
                                 int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    const char* who = "dv_rvssdw_step_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !angle_ssd || !best_heading || (reloc_below && !member_flags)) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssdw_check(c, who, n_agents, n_headings, route_of_member, win_lo, win_hi, reloc_below, channel);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rvssdw_run(c, n_agents, n_headings, route_of_member, win_lo, win_hi, reloc_below, channel, nullptr, angle_ssd, angle_view, best_heading,
                      member_flags);
}

extern "C" int dv_rvssdw_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                    const int32_t* route_of_member, const int32_t* land_of_member, const int32_t* win_lo, const int32_t* win_hi,
                                    const double* reloc_below, int channel, double* angle_ssd, int64_t* angle_view, int32_t* best_heading,
                                    uint32_t* member_flags) {
    const char* who = "dv_rvssdw_sense_step";
    if (!c) return DV_ERR_INVALID;
    if (!angle_ssd || !best_heading || !member_flags) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssdw_check(c, who, n_agents, n_headings, route_of_member, win_lo, win_hi, reloc_below, channel);
    if (!rc) rc = rvssd_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, land_of_member, channel);
    if (rc) return rc;
    return rvssdw_run(c, n_agents, n_headings, route_of_member, win_lo, win_hi, reloc_below, channel, c->rv_err, angle_ssd, angle_view,
                      best_heading, member_flags);
}
