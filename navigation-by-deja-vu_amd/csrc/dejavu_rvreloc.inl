// Re-localisation inside a windowed step (include/dejavu.h: dv_rvreloc_*): a windowed member whose best windowed familiarity lies below
// its threshold is LOST, and its step becomes the whole-route step -- decided, planned and scored on the device, in the windowed call's
// own enqueue, behind its one wait.  Everything the whole-route search needs is on the device when the windowed scores exist: the
// patches (d_sense), their byte planes (k_rv_prep), the store and the routes.  The arithmetic is dejavu_rviews.inl's own, by its own
// device functions (rv_score_tile, rv_pick_column, rv_exact_column): what differs is who wrote the plan.
//
// The host knows every member's route before the call, so the ORDER is its work: it cuts the members into consecutive groups whose
// columns fit the score buffer (rviews_slab_columns), sorts each group's members by route (stable, as rviews_plan does) and uploads
// that order with, for every sorted place, where the run of its route begins and ends.  Which of them are lost only the device knows.
// Per group, one after the other on the stream:
//   k_rvreloc_plan   ONE workgroup.  A thread a member: the largest windowed value of its row against its threshold (strict <, the
//                    doubles as they are; a member whose footprint left its landscape is never lost), lost[member], and the exclusive
//                    prefix of the lost members in sorted order (ballots within a wave, the waves' counts through LDS, a running base
//                    from one pass of 256 to the next).  Then a thread a sorted column: a lost member's column goes to
//                    col_of[prefix * A + a]; it begins a tile where its distance from the first lost column of its route is a multiple
//                    of T, and a second prefix numbers the tiles.  No atomics: every entry's place is a prefix sum, the same on every run.
//   k_rvreloc_score / _pick<0> / _exact / _pick<1>   k_rv_score / k_rv_pick / k_rv_exact on the device's plan: grids sized on the host
//                    for "every member lost", a workgroup past the device's counts returns at once.  They write the lost columns'
//                    fam and view over the windowed ones.
// k_rv_best then sets DV_RES_RELOCALISED from lost[].
namespace dv {

// The number of set `keep` among the workgroup's threads before this one, and of all 256 (ws: 4 ints of LDS).
__device__ __forceinline__ int rvreloc_scan(bool keep, int* ws, int& total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) ws[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += ws[w];
        total += ws[w];
    }
    __syncthreads();
    return before;
}

// The plan of ONE workgroup (k_rvreloc_plan's body, and k_rvssdw_plan's of dejavu_rvssdw.inl).  order, run0, run1: the group's ng
// sorted places (member; first place of its route's run; one past its last).  pm: [ng + 1].  ws: 4 ints of LDS.  NEG = 0: fam holds
// familiarities; NEG = 1: their negatives (SSDs: the familiarity is -fam, an exact negation).
// (pm, col_of: written and read here, across workgroup barriers: not __restrict__.)
template <int NEG>
__device__ __forceinline__ void rvreloc_plan(const double* __restrict__ fam, const int* __restrict__ err, const double* __restrict__ tau,
                                             const int* __restrict__ route_of, const int* __restrict__ order, const int* __restrict__ run0,
                                             const int* __restrict__ run1, int ng, int A, int T, int* __restrict__ lost, int* pm, int* col_of,
                                             RvTile* __restrict__ tiles, int* __restrict__ cnt, int* ws) {
    const int tid = (int)threadIdx.x;
    int base = 0;
    for (int m0 = 0; m0 < ng; m0 += 256) {
        const int m = m0 + tid;
        bool keep = false;
        if (m < ng) {
            const int i = order[m];
            double mx = -__builtin_inf();
            int off = 0;
            for (int a = 0; a < A; ++a) {
                const double v = NEG ? -fam[(long long)i * A + a] : fam[(long long)i * A + a];
                if (v > mx) mx = v;
                if (err && err[(long long)i * A + a]) off = 1;
            }
            keep = !off && mx < tau[i];
            lost[i] = keep ? 1 : 0;
        }
        int total;
        const int before = rvreloc_scan(keep, ws, total);
        if (m < ng) pm[m] = base + before;
        base += total;
    }
    if (tid == 0) pm[ng] = base;
    __syncthreads();
    const int ncol = ng * A;
    int tbase = 0;
    for (int s0 = 0; s0 < ncol; s0 += 256) {
        const int s = s0 + tid;
        bool start = false;
        int k = 0, ke = 0, i = 0;
        if (s < ncol) {
            const int m = s / A, a = s - m * A;
            if (pm[m + 1] > pm[m]) {                                   // (a lost member)
                i = order[m];
                k = pm[m] * A + a;
                ke = pm[run1[m]] * A;
                col_of[k] = i * A + a;
                start = (k - pm[run0[m]] * A) % T == 0;
            }
        }
        int total;
        const int t = tbase + rvreloc_scan(start, ws, total);
        if (start) tiles[t] = RvTile{k, ke - k < T ? ke - k : T, route_of[i], 0};
        tbase += total;
    }
    if (tid == 0) { cnt[0] = tbase; cnt[1] = base * A; }
}

__global__ void __launch_bounds__(256)
k_rvreloc_plan(const double* __restrict__ fam, const int* __restrict__ err, const double* __restrict__ tau, const int* __restrict__ route_of,
               const int* __restrict__ order, const int* __restrict__ run0, const int* __restrict__ run1, int ng, int A, int T,
               int* __restrict__ lost, int* pm, int* col_of, RvTile* __restrict__ tiles, int* __restrict__ cnt) {
    __shared__ int ws[4];
    rvreloc_plan<0>(fam, err, tau, route_of, order, run0, run1, ng, A, T, lost, pm, col_of, tiles, cnt, ws);
}

__global__ void __launch_bounds__(256)
k_rvreloc_score(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvTile* __restrict__ tiles,
                const int* __restrict__ col_of, const unsigned* __restrict__ prepped, const AgentW* __restrict__ wts, int A, int P, int Pw,
                int T, double* __restrict__ fast, long long lstride, const int* __restrict__ cnt) {
    if ((int)blockIdx.y >= cnt[0]) return;                             // (the whole workgroup)
    rv_score_tile(planes, routes, tiles[blockIdx.y], col_of, prepped, wts, A, P, Pw, T, fast, 0, lstride);
}

__global__ void __launch_bounds__(256)
k_rvreloc_exact(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const int* __restrict__ col_of,
                const int* __restrict__ route_of_member, const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int A,
                int P, int Pw, const int* __restrict__ marked, int force, double* __restrict__ fast, long long lstride,
                const int* __restrict__ cnt) {
    if ((int)blockIdx.y >= cnt[1]) return;
    rv_exact_column(planes, routes, col_of, route_of_member, patches, wts, A, P, Pw, marked, force, fast, 0, lstride);
}

template <int EXACT>
__global__ void __launch_bounds__(256)
k_rvreloc_pick(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const int* __restrict__ col_of,
               const int* __restrict__ route_of_member, const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int A, int P,
               int Pw, const double* __restrict__ fast, long long lstride, double delta, int* __restrict__ marked, int force,
               double* __restrict__ out_fam, long long* __restrict__ out_view, const int* __restrict__ cnt) {
    __shared__ double red[256];
    __shared__ long long redi[256];
    __shared__ int cand[kRvCandCap];
    __shared__ int n_cand;
    if ((int)blockIdx.x >= cnt[1]) return;
    rv_pick_column<EXACT>(planes, routes, col_of, route_of_member, patches, wts, A, P, Pw, fast, 0, lstride, delta, marked, force, out_fam,
                          out_view, red, redi, cand, n_cand);
}

}  // namespace dv

constexpr int kRvRelocMaxHeadings = 32768;   // a member's columns are one group's at least, and a group's columns are a grid's y

struct RvReloc {
    int N, A, T, gm, max_tiles;               // gm: members of a group at most; max_tiles: tiles of a group at most, every member lost
    long long lstride;
    std::vector<int> group_tiles;             // [n_groups]: a group's tiles with every member lost (its scoring grid)
    size_t off_tau, off_route, off_order, off_run0, off_run1;   // the call's tables within rvw_tab (bytes from its start)
};

static int rvreloc_check(dv_ctx* c, const char* who, int N, int A, const double* reloc_below) {
    if (!reloc_below) return fail(c, DV_ERR_INVALID, "%s: reloc_below is NULL", who);
    if (A > kRvRelocMaxHeadings) return fail(c, DV_ERR_INVALID, "%s: n_headings %d: a relocalising call takes %d at most", who, A, kRvRelocMaxHeadings);
    for (int i = 0; i < N; ++i)
        if (std::isnan(reloc_below[i])) return fail(c, DV_ERR_INVALID, "%s: member %d: reloc_below is NaN", who, i);
    return DV_OK;
}

// The route-sorted order and the runs of r.N members of r.A headings, in groups of r.gm consecutive members and tiles of r.T columns
// (set by the caller), behind what `tab` holds already; the thresholds and the routes beside them.
static void rvreloc_order_tables(RvReloc& r, const int32_t* route_of_member, const double* reloc_below, std::vector<unsigned char>& tab) {
    const int N = r.N, A = r.A;
    r.max_tiles = 0;
    r.group_tiles.clear();
    std::vector<int> order((size_t)N), run0((size_t)N), run1((size_t)N);
    for (int g0 = 0; g0 < N; g0 += r.gm) {
        const int ng = std::min(r.gm, N - g0);
        for (int m = 0; m < ng; ++m) order[(size_t)g0 + m] = g0 + m;
        std::stable_sort(order.begin() + g0, order.begin() + g0 + ng, [&](int a, int b) { return route_of_member[a] < route_of_member[b]; });
        int nt = 0;
        for (int m = 0; m < ng;) {
            int e = m + 1;
            while (e < ng && route_of_member[order[(size_t)g0 + e]] == route_of_member[order[(size_t)g0 + m]]) ++e;
            for (int k = m; k < e; ++k) { run0[(size_t)g0 + k] = m; run1[(size_t)g0 + k] = e; }
            nt += (int)(((long long)(e - m) * A + r.T - 1) / r.T);
            m = e;
        }
        r.group_tiles.push_back(nt);
        r.max_tiles = std::max(r.max_tiles, nt);
    }
    r.off_tau = (tab.size() + 7) / 8 * 8;
    r.off_route = r.off_tau + (size_t)N * sizeof(double);
    r.off_order = r.off_route + (size_t)N * sizeof(int);
    r.off_run0 = r.off_order + (size_t)N * sizeof(int);
    r.off_run1 = r.off_run0 + (size_t)N * sizeof(int);
    tab.resize(r.off_run1 + (size_t)N * sizeof(int), 0);
    std::memcpy(tab.data() + r.off_tau, reloc_below, (size_t)N * sizeof(double));
    std::memcpy(tab.data() + r.off_route, route_of_member, (size_t)N * sizeof(int));
    std::memcpy(tab.data() + r.off_order, order.data(), (size_t)N * sizeof(int));
    std::memcpy(tab.data() + r.off_run0, run0.data(), (size_t)N * sizeof(int));
    std::memcpy(tab.data() + r.off_run1, run1.data(), (size_t)N * sizeof(int));
}

// The SADS call's groups (what the score buffer holds) and tile width, and their tables behind the windowed call's weights and windows.
static void rvreloc_tables(const dv_ctx* c, RvReloc& r, int N, int A, const int32_t* route_of_member, const double* reloc_below,
                           std::vector<unsigned char>& tab) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4;
    r.N = N; r.A = A;
    r.T = std::min(kRvTileMax, kRvLdsBytes / (3 * Pw * 4) / kRvBlock * kRvBlock);          // rviews_plan's rule
    r.lstride = ((long long)c->rv_lmax + 63) / 64 * 64;
    r.gm = std::min(N, std::max(1, rviews_slab_columns(c, r.lstride) / A));
    rvreloc_order_tables(r, route_of_member, reloc_below, tab);
}

// What the device writes of a plan (rvw_plan): lost[N], pm[gm + 1], cnt[2], col_of[gm A], tiles[max_tiles].
struct RvRelocDev { int* lost; int* pm; int* cnt; int* col_of; RvTile* tiles; };

static RvRelocDev rvreloc_dev(unsigned char* plan, const RvReloc& r) {
    RvRelocDev d;
    d.lost = reinterpret_cast<int*>(plan);
    d.pm = d.lost + r.N;
    d.cnt = d.pm + r.gm + 1;
    d.col_of = d.cnt + 2;
    size_t tiles_at = ((size_t)r.N + r.gm + 3 + (size_t)r.gm * r.A) * sizeof(int);
    tiles_at = (tiles_at + 15) / 16 * 16;
    d.tiles = reinterpret_cast<RvTile*>(plan + tiles_at);
    return d;
}

static size_t rvreloc_plan_bytes(const RvReloc& r) {
    const size_t plan = ((size_t)r.N + r.gm + 3 + (size_t)r.gm * r.A) * sizeof(int);
    return (plan + 15) / 16 * 16 + (size_t)r.max_tiles * sizeof(RvTile);
}

static int rvreloc_buffers(dv_ctx* c, const RvReloc& r) {
    const size_t gcols = (size_t)r.gm * r.A;
    int rc = grow_buffer(c, c->rvw_plan, c->rvw_plan_cap, rvreloc_plan_bytes(r));
    if (!rc) rc = grow_buffer(c, c->rv_fast, c->rv_fast_cap, gcols * (size_t)r.lstride * sizeof(double));
    if (!rc) rc = grow_buffer(c, c->rv_marked, c->rv_marked_cap, gcols * sizeof(int));
    return rc;
}

// Behind the windowed scoring launches of the call: per group the plan and the whole-route scoring of its lost columns.
static int rvreloc_enqueue(dv_ctx* c, const RvReloc& r, bool exact, const int* err, const AgentW* wts, double* d_fam, long long* d_view) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4, A = r.A;
    const RvRelocDev d = rvreloc_dev(c->rvw_plan, r);
    const double* tau = reinterpret_cast<const double*>(c->rvw_tab.dev + r.off_tau);
    const int* route_of = reinterpret_cast<const int*>(c->rvw_tab.dev + r.off_route);
    const int* order = reinterpret_cast<const int*>(c->rvw_tab.dev + r.off_order);
    const int* run0 = reinterpret_cast<const int*>(c->rvw_tab.dev + r.off_run0);
    const int* run1 = reinterpret_cast<const int*>(c->rvw_tab.dev + r.off_run1);
    const unsigned chunks = (unsigned)((c->rv_lmax + 255) / 256);
    const size_t lds = (size_t)r.T * 3 * Pw * 4;
    const int vpw = std::max(1, 4 / (r.T / kRvBlock));                  // as rviews_run
    const unsigned vchunks = (unsigned)(((c->rv_lmax + 63) / 64 + vpw - 1) / vpw);
    for (size_t g = 0; g < r.group_tiles.size(); ++g) {
        const int g0 = (int)g * r.gm, ng = std::min(r.gm, r.N - g0);
        const unsigned n = (unsigned)(ng * A);
        hipLaunchKernelGGL(k_rvreloc_plan, dim3(1), dim3(256), 0, c->stream, d_fam, err, tau, route_of, order + g0, run0 + g0, run1 + g0, ng, A, r.T,
                           d.lost, d.pm, d.col_of, d.tiles, d.cnt);
        if (!exact) {
            hipLaunchKernelGGL(k_rvreloc_score, dim3(vchunks, (unsigned)r.group_tiles[g]), dim3(256), lds, c->stream, c->rv_planes, c->rv_routes,
                               d.tiles, d.col_of, c->rv_prep, wts, A, P, Pw, r.T, c->rv_fast, r.lstride, d.cnt);
            hipLaunchKernelGGL(k_rvreloc_pick<0>, dim3(n), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, d.col_of, route_of, c->d_sense, wts,
                               A, P, Pw, c->rv_fast, r.lstride, c->rv_delta, c->rv_marked, 0, d_fam, d_view, d.cnt);
        }
        hipLaunchKernelGGL(k_rvreloc_exact, dim3(chunks, n), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, d.col_of, route_of, c->d_sense, wts,
                           A, P, Pw, c->rv_marked, exact ? 1 : 0, c->rv_fast, r.lstride, d.cnt);
        hipLaunchKernelGGL(k_rvreloc_pick<1>, dim3(n), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, d.col_of, route_of, c->d_sense, wts, A, P,
                           Pw, c->rv_fast, r.lstride, c->rv_delta, c->rv_marked, exact ? 1 : 0, d_fam, d_view, d.cnt);
        HIP_TRY(c, hipGetLastError());
    }
    return DV_OK;
}
