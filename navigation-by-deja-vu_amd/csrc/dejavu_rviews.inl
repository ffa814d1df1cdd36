// Route view store (include/dejavu.h: dv_rviews_*): the sensed views of R training routes side by side as raw HSV bytes, and a step
// that scores every member's headings against the views of ITS OWN route only -- the perfect-memory model (sads_hsv) for ensembles of
// trials that differ in their training route and their landscape.  It stands beside the library (set_library, k_sad_*, k_finish):
// nothing here reads or writes the library's buffers, its layouts or its step state, and nothing there reads the store.
//
// Store.  Route r is views [first[r], first[r+1]) of the call that made the store, at least 2 each.  A route's views are cut into
// groups of 64 (the last group of a route is padded; a group never holds views of two routes), and a group is three byte planes
// (H, S, V) of Pw = ceil(P / 4) dwords per view, lane-interleaved:
//     planes[((g * 3 + plane) * Pw + q) * 64 + lane]  =  bytes 4q .. 4q+3 of `plane` of view lane of group g     (0 beyond P)
// so that the 64 lanes of a wave, a view each, load consecutive dwords.  The layout depends on neither the data nor a weight.
//
// Step.  Columns are (member, heading) pairs.  The host sorts the members by route (stable, so the order within a route is the
// caller's) and cuts the sorted columns into slabs (what the score buffer holds) and, inside a slab, into tiles of at most kRvTileMax
// columns of ONE route.  Per slab:
//   k_rv_prep    the call's patches as byte planes (dwords), once per call.
//   k_rv_score   workgroup = (1, 2 or 4 groups of 64 views of the tile's route, one tile): the tile's patches go to LDS as byte planes,
//                a wave takes kRvBlock columns of the tile and one view group, a lane keeps those columns' two integer sums against
//                its view (byte SADs and byte dot products, any hue, any level), and writes the fast score
//                P - (whs S_hs + wv S_v) / 255 of every (column, view) to fast[column][view].
//   k_rv_pick    workgroup = column: the column's fast maximum, every view within 2 delta of it (at most kRvCandCap; more: the
//                column is marked for the exact-all pass), each candidate scored again as the reference's sequential double sum, the
//                largest exact value and the first view that attains it.
//   k_rv_exact   the sequential double sum of every view of the marked columns (all columns in exact mode) into fast[][], and
//   k_rv_pick<1> the maximum and its first view of those rows.
// k_rv_best then takes every member's first maximum over its columns (np.argmax) and its off-landscape flag.  There are no atomics
// on doubles and no order among workgroups matters: a column's result is a maximum and a least index.
namespace dv {

constexpr int kRvBlock = 4;                  // columns whose sums a lane keeps at a time
constexpr int kRvTileMax = 16;               // columns of a tile at most (a multiple of kRvBlock)
constexpr int kRvLdsBytes = 48 * 1024;       // LDS budget of a tile's patches
constexpr int kRvCandCap = 256;              // candidates of a column that k_rv_pick scores itself
constexpr int kRvMaxPixels = kRvLdsBytes / (3 * kRvBlock);   // 4096: kRvBlock patches must fit the budget

struct RvGroup { long long v0; int n; int pad; };        // a group of the store: its first view in the call's views, its views (1..64)
struct RvRoute { long long g0; int len; int pad; };      // a route: its first group, its views
struct RvTile { int s0, n, route, pad; };                // sorted columns [s0, s0 + n) of one route

__device__ __forceinline__ unsigned rv_pack4(const unsigned char* __restrict__ p, int px, int P, int plane) {
    unsigned w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (px + k < P) w |= (unsigned)p[(long long)(px + k) * 3 + plane] << (8 * k);
    return w;
}

// raw: uint8[n][P][3] -> the store's planes; one thread per dword.
__global__ void k_rv_planes(const unsigned char* __restrict__ raw, const RvGroup* __restrict__ groups, long long n_groups, int P, int Pw,
                            unsigned* __restrict__ planes) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_groups * 3 * Pw * 64) return;
    const int lane = (int)(t & 63);
    const int q = (int)((t >> 6) % Pw);
    const int plane = (int)(((t >> 6) / Pw) % 3);
    const RvGroup g = groups[(t >> 6) / ((long long)Pw * 3)];
    planes[t] = lane < g.n ? rv_pack4(raw + (g.v0 + lane) * (long long)P * 3, 4 * q, P, plane) : 0u;
}

// raw patches uint8[C][P][3] -> byte planes [C][3][Pw] dwords (the caller's column order); one thread per dword.
__global__ void k_rv_prep(const unsigned char* __restrict__ patches, long long C, int P, int Pw, unsigned* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C * 3 * Pw) return;
    const int q = (int)(t % Pw), plane = (int)((t / Pw) % 3);
    out[t] = rv_pack4(patches + (t / ((long long)Pw * 3)) * P * 3, 4 * q, P, plane);
}

// Workgroup = (vpw groups of 64 views of the tile's route) x (one tile): with T the call's tile width, the 4 waves are T / 4 column
// blocks times vpw = 4 / (T / 4) view groups (T = 16: 1 group, 8: 2, 4: 4; T = 12: 1 group and an idle wave).  A lane holds one
// view's dwords and the two sums of its wave's kRvBlock columns.  (The body is k_rv_score's and, with a plan the device wrote,
// k_rvreloc_score's of dejavu_rvreloc.inl: one statement of the sums.)
__device__ __forceinline__ void rv_score_tile(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvTile tile,
                                              const int* __restrict__ col_of, const unsigned* __restrict__ prepped,
                                              const AgentW* __restrict__ wts, int A, int P, int Pw, int T, double* __restrict__ fast, int slab_s0,
                                              long long lstride) {
    extern __shared__ unsigned rv_lds[];                              // [round4(n)][3][Pw]
    const RvRoute rt = routes[tile.route];
    const int ncb = T / kRvBlock, vpw = 4 / ncb > 0 ? 4 / ncb : 1;
    if ((long long)blockIdx.x * vpw * 64 >= rt.len) return;           // (the whole workgroup)
    const int npad = (tile.n + kRvBlock - 1) / kRvBlock * kRvBlock;
    for (int i = threadIdx.x; i < npad * 3 * Pw; i += 256) {
        const int k = i / (3 * Pw);
        rv_lds[i] = k < tile.n ? prepped[(long long)col_of[tile.s0 + k] * 3 * Pw + (i - k * 3 * Pw)] : 0u;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k0 = (wave % ncb) * kRvBlock;
    const long long gl = (long long)blockIdx.x * vpw + wave / ncb;
    if (wave / ncb >= vpw || k0 >= tile.n || gl * 64 >= rt.len) return;
    const long long f = gl * 64 + lane;
    const unsigned* __restrict__ base = planes + (rt.g0 + gl) * 3 * Pw * 64 + lane;
    int hs[kRvBlock], sv[kRvBlock];
#pragma unroll
    for (int j = 0; j < kRvBlock; ++j) hs[j] = sv[j] = 0;
    const unsigned* __restrict__ pl = rv_lds + (long long)k0 * 3 * Pw;
#pragma unroll 2
    for (int q = 0; q < Pw; ++q) {
        const unsigned H = base[(long long)q * 64], S = base[(long long)(Pw + q) * 64], V = base[(long long)(2 * Pw + q) * 64];
#pragma unroll
        for (int j = 0; j < kRvBlock; ++j) {
            const unsigned ph = pl[(j * 3) * Pw + q], ps = pl[(j * 3 + 1) * Pw + q], pv = pl[(j * 3 + 2) * Pw + q];
            // the pixels whose hues differ add S_s + S_f (a dot product with their 0x01 bytes), the others |S_s - S_f| (the differing
            // pixels' bytes are set to 0xff in both operands and add nothing)
            const unsigned x = ph ^ H;
            const unsigned t = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
            const unsigned one = t >> 7, ne = (t - one) | t;
            unsigned h = __builtin_amdgcn_udot4(ps, one, (unsigned)hs[j], false);
            h = __builtin_amdgcn_udot4(S, one, h, false);
            hs[j] = (int)__builtin_amdgcn_sad_u8(ps | ne, S | ne, h);
            sv[j] = (int)__builtin_amdgcn_sad_u8(pv, V, (unsigned)sv[j]);
        }
    }
    if (f < rt.len) {
#pragma unroll
        for (int j = 0; j < kRvBlock; ++j)
            if (k0 + j < tile.n) {
                const int s = tile.s0 + k0 + j;
                const AgentW w = wts[col_of[s] / A];
                fast[(long long)(s - slab_s0) * lstride + f] = (double)P - (w.whs * (double)hs[j] + w.wv * (double)sv[j]) / 255.0;
            }
    }
}

__global__ void __launch_bounds__(256)
k_rv_score(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvTile* __restrict__ tiles,
           const int* __restrict__ col_of, const unsigned* __restrict__ prepped, const AgentW* __restrict__ wts, int A, int P, int Pw, int T,
           double* __restrict__ fast, int slab_s0, long long lstride) {
    rv_score_tile(planes, routes, tiles[blockIdx.y], col_of, prepped, wts, A, P, Pw, T, fast, slab_s0, lstride);
}

// The reference's value of one (patch, view): per-pixel terms in its operation order, added in pixel order (util.pyx:44-73).
__device__ __forceinline__ double rv_exact_view(const unsigned* __restrict__ base, const unsigned char* __restrict__ patch, int P, int Pw,
                                                double cw, double wv) {
    double diff = 0.0;
    for (int q = 0; q < Pw; ++q) {
        const unsigned H = base[(long long)q * 64], S = base[(long long)(Pw + q) * 64], V = base[(long long)(2 * Pw + q) * 64];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int px = 4 * q + k;
            if (px < P) {
                const int hf = (int)((H >> (8 * k)) & 0xffu), sf = (int)((S >> (8 * k)) & 0xffu), vf = (int)((V >> (8 * k)) & 0xffu);
                const int hp = patch[px * 3], sp = patch[px * 3 + 1], vp = patch[px * 3 + 2];
                const int hsv = hp == hf ? abs(sp - sf) : sp + sf;
                diff += px_term(hsv, abs(vp - vf), cw, wv);
            }
        }
    }
    return (double)P - diff;
}

__device__ __forceinline__ const unsigned* rv_view_base(const unsigned* __restrict__ planes, const RvRoute& rt, long long f, int Pw) {
    return planes + (rt.g0 + (f >> 6)) * 3 * Pw * 64 + (f & 63);
}

// Every view of the marked columns of a slab (force: of all its columns); grid = (256-view chunks, the slab's columns).  (The body is
// k_rv_exact's and k_rvreloc_exact's.)
__device__ __forceinline__ void rv_exact_column(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes,
                                                const int* __restrict__ col_of, const int* __restrict__ route_of_member,
                                                const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int A, int P, int Pw,
                                                const int* __restrict__ marked, int force, double* __restrict__ fast, int slab_s0,
                                                long long lstride) {
    const int s = slab_s0 + blockIdx.y;
    if (!force && !marked[s]) return;
    const int oc = col_of[s];
    const RvRoute rt = routes[route_of_member[oc / A]];
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= rt.len) return;
    const AgentW w = wts[oc / A];
    fast[(long long)blockIdx.y * lstride + f] = rv_exact_view(rv_view_base(planes, rt, f, Pw), patches + (long long)oc * P * 3, P, Pw, w.cw, w.wv);
}

__global__ void __launch_bounds__(256)
k_rv_exact(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const int* __restrict__ col_of,
           const int* __restrict__ route_of_member, const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int A, int P,
           int Pw, const int* __restrict__ marked, int force, double* __restrict__ fast, int slab_s0, long long lstride) {
    rv_exact_column(planes, routes, col_of, route_of_member, patches, wts, A, P, Pw, marked, force, fast, slab_s0, lstride);
}

// The largest of v over the workgroup's 256 threads and the least idx among the threads that hold it (red, redi: 256 entries each).
__device__ __forceinline__ void rv_block_max(double& v, long long& idx, double* red, long long* redi) {
    red[threadIdx.x] = v;
    redi[threadIdx.x] = idx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double ov = red[threadIdx.x + o];
            const long long oi = redi[threadIdx.x + o];
            if (ov > red[threadIdx.x] || (ov == red[threadIdx.x] && oi < redi[threadIdx.x])) { red[threadIdx.x] = ov; redi[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    v = red[0];
    idx = redi[0];
    __syncthreads();
}

// EXACT = 0: the rows hold fast scores (see the head of the file).  EXACT = 1: the rows of the marked columns (force: of all) hold the
// reference's values: the maximum and its first view.  (The body is k_rv_pick's and k_rvreloc_pick's; red, redi, cand, n_cand: the
// kernel's static LDS.)
template <int EXACT>
__device__ __forceinline__ void rv_pick_column(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes,
                                               const int* __restrict__ col_of, const int* __restrict__ route_of_member,
                                               const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int A, int P, int Pw,
                                               const double* __restrict__ fast, int slab_s0, long long lstride, double delta,
                                               int* __restrict__ marked, int force, double* __restrict__ out_fam, long long* __restrict__ out_view,
                                               double* red, long long* redi, int* cand, int& n_cand) {
    const int s = slab_s0 + blockIdx.x;
    if (EXACT && !force && !marked[s]) return;
    const int oc = col_of[s];
    const RvRoute rt = routes[route_of_member[oc / A]];
    const double* __restrict__ row = fast + (long long)blockIdx.x * lstride;
    const long long kNone = 0x7fffffffffffffffll;
    double m = -__builtin_inf();
    long long at = kNone;
    for (long long f = threadIdx.x; f < rt.len; f += 256)
        if (row[f] > m) { m = row[f]; at = f; }                        // (a thread's views ascend: its first maximum)
    rv_block_max(m, at, red, redi);
    if (EXACT) {
        if (threadIdx.x == 0) { out_fam[oc] = m; out_view[oc] = at; }
        return;
    }
    if (threadIdx.x == 0) n_cand = 0;
    __syncthreads();
    const double floor_ = m - 2.0 * delta;
    for (long long f = threadIdx.x; f < rt.len; f += 256)
        if (row[f] >= floor_) {
            const int slot = atomicAdd(&n_cand, 1);
            if (slot < kRvCandCap) cand[slot] = (int)f;
        }
    __syncthreads();
    const int n = n_cand;
    if (n > kRvCandCap) {                                              // (the list's order is the only thing that varies: not read)
        if (threadIdx.x == 0) marked[s] = 1;
        return;
    }
    double v = -__builtin_inf();
    long long vf = kNone;
    if ((int)threadIdx.x < n) {
        const AgentW w = wts[oc / A];
        vf = cand[threadIdx.x];
        v = rv_exact_view(rv_view_base(planes, rt, vf, Pw), patches + (long long)oc * P * 3, P, Pw, w.cw, w.wv);
    }
    rv_block_max(v, vf, red, redi);
    if (threadIdx.x == 0) { marked[s] = 0; out_fam[oc] = v; out_view[oc] = vf; }
}

template <int EXACT>
__global__ void __launch_bounds__(256)
k_rv_pick(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const int* __restrict__ col_of,
          const int* __restrict__ route_of_member, const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int A, int P, int Pw,
          const double* __restrict__ fast, int slab_s0, long long lstride, double delta, int* __restrict__ marked, int force,
          double* __restrict__ out_fam, long long* __restrict__ out_view) {
    __shared__ double red[256];
    __shared__ long long redi[256];
    __shared__ int cand[kRvCandCap];
    __shared__ int n_cand;
    rv_pick_column<EXACT>(planes, routes, col_of, route_of_member, patches, wts, A, P, Pw, fast, slab_s0, lstride, delta, marked, force, out_fam,
                          out_view, red, redi, cand, n_cand);
}

// A member's first maximum over its A columns (np.argmax) and its flags: err is a word per column (nullptr: patches were uploaded),
// lost a word per member (nullptr but in a relocalising call: dejavu_rvreloc.inl).
__global__ void k_rv_best(const double* __restrict__ fam, const int* __restrict__ err, const int* __restrict__ lost, int n, int A,
                          int* __restrict__ best, unsigned* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int b = 0, off = 0;
    for (int a = 0; a < A; ++a) {
        if (fam[(long long)i * A + a] > fam[(long long)i * A + b]) b = a;
        if (err && err[(long long)i * A + a]) off = 1;
    }
    best[i] = off ? -1 : b;
    flags[i] = off ? 16u : lost && lost[i] ? 32u : 0u;                 // DV_RES_SENSE_ERROR, DV_RES_RELOCALISED
}

// scene_familiarity: per view of the member's route the least exact value over the member's A headings (strict <, from +inf: :287,
// :301-303); grid = (256-view chunks, members); out is ragged, member i's row begins at row0[i].
__global__ void __launch_bounds__(256)
k_rv_scene(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const int* __restrict__ route_of_member,
           const long long* __restrict__ row0, const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int A, int P, int Pw,
           double* __restrict__ out) {
    const int i = blockIdx.y;
    const RvRoute rt = routes[route_of_member[i]];
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= rt.len) return;
    const AgentW w = wts[i];
    const unsigned* base = rv_view_base(planes, rt, f, Pw);
    double m = __builtin_inf();
    for (int a = 0; a < A; ++a) {
        const double v = rv_exact_view(base, patches + ((long long)i * A + a) * P * 3, P, Pw, w.cw, w.wv);
        if (v < m) m = v;
    }
    out[row0[i] + f] = m;
}

}  // namespace dv

static void rviews_free(dv_ctx* c) {
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->rv_planes); F(c->rv_routes); F(c->rv_fast); F(c->rv_marked); F(c->rv_out); F(c->rv_err); F(c->rv_scene); F(c->rv_prep); F(c->rvw_plan);
    c->rvw_plan_cap = 0;
    c->rv_fast_cap = c->rv_marked_cap = c->rv_out_cap = c->rv_err_cap = c->rv_scene_cap = c->rv_prep_cap = 0;
    c->rv_first.clear();
    table_free(c->rv_tab);
    table_free(c->rvw_tab);
    c->rv_h = c->rv_w = 0;
    c->rv_lmax = 0;
    c->rv_bytes = 0;
    ++c->rv_gen;
}

static int rviews_need(dv_ctx* c, const char* who) {
    if (!c->rv_planes) return fail(c, DV_ERR_STATE, "%s: no route views (dv_rviews_set_u8 or dv_rviews_set_from_poses first)", who);
    return DV_OK;
}

static int rviews_check_first(dv_ctx* c, const char* who, const int64_t* first, int n_routes) {
    if (!first) return fail(c, DV_ERR_INVALID, "%s: first is NULL", who);
    if (n_routes < 1) return fail(c, DV_ERR_INVALID, "%s: n_routes %d < 1", who, n_routes);
    if (first[0] != 0) return fail(c, DV_ERR_INVALID, "%s: first[0] = %lld, not 0", who, (long long)first[0]);
    for (int r = 0; r < n_routes; ++r)
        if (first[r + 1] - first[r] < 2 || first[r + 1] - first[r] > 0x7fffffff)
            return fail(c, DV_ERR_INVALID, "%s: first[%d] = %lld: route %d would hold %lld views (a route holds at least 2)", who, r + 1,
                        (long long)first[r + 1], r, (long long)(first[r + 1] - first[r]));
    return DV_OK;
}

static int rviews_check_shape(dv_ctx* c, const char* who, int h, int w) {
    if (h < 1 || w < 1 || (long long)h * w > kRvMaxPixels)
        return fail(c, DV_ERR_INVALID, "%s: views of %d x %d: h and w >= 1 and h * w <= %d", who, h, w, kRvMaxPixels);
    return DV_OK;
}

// The store of the n = first[n_routes] views that lie raw in d_raw (uint8[n][h][w][3]): built beside the old one, in place when complete.
static int rviews_build(dv_ctx* c, const char* who, const unsigned char* d_raw, const int64_t* first, int n_routes, int h, int w) {
    const int P = h * w, Pw = (P + 3) / 4;
    std::vector<RvRoute> routes((size_t)n_routes);
    std::vector<RvGroup> groups;
    int lmax = 0;
    for (int r = 0; r < n_routes; ++r) {
        const int len = (int)(first[r + 1] - first[r]);
        routes[(size_t)r] = RvRoute{(long long)groups.size(), len, 0};
        for (int v = 0; v < len; v += 64) groups.push_back(RvGroup{(long long)first[r] + v, std::min(64, len - v), 0});
        lmax = std::max(lmax, len);
    }
    const size_t dwords = groups.size() * 3 * (size_t)Pw * 64;
    unsigned* d = nullptr;
    RvRoute* t = nullptr;
    RvGroup* g = nullptr;
    hipError_t e = hipMalloc((void**)&d, dwords * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&t, routes.size() * sizeof(RvRoute));
    if (e == hipSuccess) e = hipMalloc((void**)&g, groups.size() * sizeof(RvGroup));
    if (e == hipSuccess) e = hipMemcpyAsync(t, routes.data(), routes.size() * sizeof(RvRoute), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(g, groups.data(), groups.size() * sizeof(RvGroup), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rv_planes, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, c->stream, d_raw, g, (long long)groups.size(), P, Pw, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (g) (void)hipFree(g);
    if (e != hipSuccess) {                                              // the old store stays as it was
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        if (t) (void)hipFree(t);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "%s: %d routes of %lld views: %s", who, n_routes,
                    (long long)first[n_routes], hipGetErrorString(e));
    }
    if (c->rv_planes) (void)hipFree(c->rv_planes);
    if (c->rv_routes) (void)hipFree(c->rv_routes);
    c->rv_planes = d;
    c->rv_routes = t;
    c->rv_first.assign(first, first + n_routes + 1);
    c->rv_h = h;
    c->rv_w = w;
    c->rv_lmax = lmax;
    c->rv_bytes = (long long)(dwords * 4);
    c->rv_delta = 4.0 * (P + 8.0) * std::ldexp(1.0, -53) * P;           // alloc_library's c->delta
    c->rv_tab.host.clear();
    ++c->rv_gen;                                                        // (what dejavu_rvssd.inl keeps of the old store is void)
    return DV_OK;
}

struct RvRaw {                               // a call's own device buffer (hipFree waits for what still reads it)
    unsigned char* p = nullptr;
    ~RvRaw() { if (p) (void)hipFree(p); }
};

extern "C" int dv_rviews_set_u8(dv_ctx* c, const uint8_t* views, const int64_t* first, int n_routes, int h, int w) {
    if (!c) return DV_ERR_INVALID;
    if (!views) return fail(c, DV_ERR_INVALID, "dv_rviews_set_u8: views is NULL");
    int rc = rviews_check_first(c, "dv_rviews_set_u8", first, n_routes);
    if (!rc) rc = rviews_check_shape(c, "dv_rviews_set_u8", h, w);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)first[n_routes] * h * w * 3;
    RvRaw raw;                                                          // (the raw views: this call's, freed when the planes are made)
    HIP_TRY(c, hipMalloc((void**)&raw.p, bytes));
    HIP_TRY(c, hipMemcpyAsync(raw.p, views, bytes, hipMemcpyHostToDevice, c->stream));
    return rviews_build(c, "dv_rviews_set_u8", raw.p, first, n_routes, h, w);
}

// Sense the C poses resident in d_poses into d_out, a word per pose in rv_err: on the engine's landscape, or (per > 0) pose v on
// landscape ld_of[v / per] of the live set (the table checked and uploaded by the caller).
static int rviews_enqueue_sense(dv_ctx* c, long long C, int per, unsigned char* d_out) {
    int rc = grow_buffer(c, c->rv_err, c->rv_err_cap, (size_t)C * sizeof(int));
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->rv_err, 0, (size_t)C * sizeof(int), c->stream));
    if (per > 0) return lands_launch_sense(c, 0, 0, per, C, d_out, c->rv_err);
    const long long total = C * c->sensor.sh * c->sensor.sw;
    hipLaunchKernelGGL(k_sense_each, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->d_land, c->d_poses, (int)C, c->sensor, c->d_lut,
                       d_out, c->rv_err);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

static int rviews_check_poses(dv_ctx* c, const char* who, long long C) {
    if (!c->have_sensor) return fail(c, DV_ERR_STATE, "sensor not configured");
    if (C * c->sensor.sh * c->sensor.sw > 0x7fffffffll * 256 || C > 0x7fffffff)
        return fail(c, DV_ERR_INVALID, "%s: %lld poses are more than one call senses", who, C);
    return DV_OK;
}

extern "C" int dv_rviews_set_from_poses(dv_ctx* c, const double* x, const double* y, const double* angle, int64_t n, const int64_t* first,
                                        int n_routes, const int32_t* land_of_view, uint8_t* out_views) {
    const char* who = "dv_rviews_set_from_poses";
    if (!c) return DV_ERR_INVALID;
    if (!x || !y || !angle) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rviews_check_first(c, who, first, n_routes);
    if (rc) return rc;
    if (first[n_routes] != n) return fail(c, DV_ERR_INVALID, "%s: first[%d] = %lld, but n = %lld views", who, n_routes, (long long)first[n_routes], (long long)n);
    rc = rviews_check_poses(c, who, n);
    if (!rc) rc = rviews_check_shape(c, who, c->sensor.sh, c->sensor.sw);
    if (!rc) rc = land_of_view ? lands_check(c, who, "land_of_view", land_of_view, n) : noise_need_lands(c, who);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * c->sensor.sh * c->sensor.sw * 3;
    RvRaw raw;                                                          // (the raw views: this call's, freed when the planes are made)
    HIP_TRY(c, hipMalloc((void**)&raw.p, bytes));
    if (land_of_view) rc = lands_upload(c, land_of_view, n);
    if (!rc) rc = upload_member_poses(c, x, y, angle, (int)n, 1);
    if (!rc) rc = rviews_enqueue_sense(c, n, land_of_view ? 1 : 0, raw.p);
    if (rc) return rc;
    std::vector<int> err((size_t)n);
    HIP_TRY(c, hipMemcpyAsync(err.data(), c->rv_err, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (out_views) HIP_TRY(c, hipMemcpyAsync(out_views, raw.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t v = 0; v < n; ++v)
        if (err[(size_t)v]) {
            if (land_of_view) {
                const int l = land_of_view[v];
                return fail(c, DV_ERR_INDEX, "%s: the sensor footprint of view %lld reaches past the end of its landscape %d (%d x %d) (index out of bounds)",
                            who, (long long)v, l, c->ld_rows[(size_t)l], c->ld_cols[(size_t)l]);
            }
            return fail(c, DV_ERR_INDEX, "%s: the sensor footprint of view %lld reaches past the end of the landscape (index out of bounds)", who, (long long)v);
        }
    return rviews_build(c, who, raw.p, first, n_routes, c->sensor.sh, c->sensor.sw);
}

extern "C" int dv_rviews_clear(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rviews_free(c);
    return DV_OK;
}

extern "C" int dv_rviews_info(dv_ctx* c, int* n_routes, int64_t* first, int* h, int* w, int64_t* bytes) {
    if (!c) return DV_ERR_INVALID;
    if (n_routes) *n_routes = c->rv_first.empty() ? 0 : (int)c->rv_first.size() - 1;
    if (first) std::copy(c->rv_first.begin(), c->rv_first.end(), first);
    if (h) *h = c->rv_h;
    if (w) *w = c->rv_w;
    if (bytes) *bytes = (int64_t)c->rv_bytes;
    return DV_OK;
}

// ---- a step ----------------------------------------------------------------------------------------------------------------------------------
// The tables of a call, checked entry by entry before anything of the call reaches the device.
static int rviews_check_tables(dv_ctx* c, const char* who, int N, int A, const int32_t* route_of_member, const double* chem_weights) {
    if (N < 1 || A < 1) return fail(c, DV_ERR_INVALID, "%s: n_agents %d and n_headings %d must be >= 1", who, N, A);
    if ((long long)N * A > 0x7fffffffll / 4) return fail(c, DV_ERR_INVALID, "%s: %d x %d columns are more than one call takes", who, N, A);
    if (!route_of_member || !chem_weights) return fail(c, DV_ERR_INVALID, "%s: NULL table", who);
    int rc = rviews_need(c, who);
    if (rc) return rc;
    rc = index_check(c, who, "route_of_member", route_of_member, N, (int)c->rv_first.size() - 1, "n_routes");
    if (rc) return rc;
    for (int i = 0; i < N; ++i)
        if (!(chem_weights[i] >= 0.0 && chem_weights[i] <= 1.0))
            return fail(c, DV_ERR_INVALID, "%s: chem_weights[%d] = %g outside [0, 1]", who, i, chem_weights[i]);
    return DV_OK;
}

struct RvPlan {
    int N, A, C, T, slab;                     // T: columns of a tile at most; slab: columns of a slab at most
    long long lstride;
    std::vector<int> slab_tile0;              // [n_slabs + 1]: a slab's tiles
    // the device's tables within rv_tab (bytes from its start)
    size_t off_wts, off_tiles, off_col, off_route, off_row0;
};

static int rviews_slab_columns(const dv_ctx* c, long long lstride) {
    long long cols = std::max(1ll, (64ll << 20) / (lstride * 8));
    if (c->rv_slab_env >= 1) cols = c->rv_slab_env;                     // (DEJAVU_RVIEWS_SLAB at dv_create: slab edges at small sizes, tests)
    return (int)std::min(cols, 32768ll);                                 // (a slab's columns, and so its tiles, are a grid's y)
}

// Sort the members by route, cut the sorted columns into slabs and tiles, and bring the device's tables up to date (one copy, and
// none when they hold the same already).  row0 (may be nullptr): the ragged rows of a scene call.
static int rviews_plan(dv_ctx* c, RvPlan& p, int N, int A, const int32_t* route_of_member, const double* chem_weights, const long long* row0) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4;
    p.N = N; p.A = A; p.C = N * A;
    p.T = std::min(kRvTileMax, kRvLdsBytes / (3 * Pw * 4) / kRvBlock * kRvBlock);
    p.lstride = ((long long)c->rv_lmax + 63) / 64 * 64;
    p.slab = std::min(p.C, rviews_slab_columns(c, p.lstride));
    std::vector<int> order((size_t)N);
    for (int i = 0; i < N; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return route_of_member[a] < route_of_member[b]; });
    std::vector<int> col_of((size_t)p.C);
    for (int m = 0; m < N; ++m)
        for (int a = 0; a < A; ++a) col_of[(size_t)m * A + a] = order[(size_t)m] * A + a;
    std::vector<RvTile> tiles;
    p.slab_tile0.assign(1, 0);
    for (int s0 = 0; s0 < p.C; s0 += p.slab) {
        const int s1 = std::min(p.C, s0 + p.slab);
        for (int s = s0; s < s1;) {
            const int r = route_of_member[col_of[(size_t)s] / A];
            int e = s + 1;
            while (e < s1 && e - s < p.T && route_of_member[col_of[(size_t)e] / A] == r) ++e;
            tiles.push_back(RvTile{s, e - s, r, 0});
            s = e;
        }
        p.slab_tile0.push_back((int)tiles.size());
    }
    p.off_wts = 0;
    p.off_tiles = p.off_wts + (size_t)N * sizeof(AgentW);
    p.off_row0 = p.off_tiles + tiles.size() * sizeof(RvTile);
    p.off_col = p.off_row0 + (size_t)N * sizeof(long long);
    p.off_route = p.off_col + (size_t)p.C * sizeof(int);
    std::vector<unsigned char> tab(p.off_route + (size_t)N * sizeof(int), 0);
    AgentW* w = reinterpret_cast<AgentW*>(tab.data() + p.off_wts);
    for (int i = 0; i < N; ++i) w[i] = AgentW{chem_weights[i], 0.5 * chem_weights[i], 1 - chem_weights[i], 0.0};   // as alloc_library computes its own
    std::memcpy(tab.data() + p.off_tiles, tiles.data(), tiles.size() * sizeof(RvTile));
    if (row0) std::memcpy(tab.data() + p.off_row0, row0, (size_t)N * sizeof(long long));
    std::memcpy(tab.data() + p.off_col, col_of.data(), col_of.size() * sizeof(int));
    std::memcpy(tab.data() + p.off_route, route_of_member, (size_t)N * sizeof(int));
    return table_upload(c, c->rv_tab, tab.data(), tab.size());
}

// Score the C columns whose patches lie in d_sense (uint8[C][P][3], the caller's order); err: a word per column, or nullptr.
static int rviews_run(dv_ctx* c, const RvPlan& p, bool exact, const int* err, double* angle_fam, int64_t* angle_view, int32_t* best_heading,
                      uint32_t* member_flags) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4, A = p.A;
    int rc = grow_buffer(c, c->rv_fast, c->rv_fast_cap, (size_t)p.slab * (size_t)p.lstride * sizeof(double));
    if (!rc) rc = grow_buffer(c, c->rv_marked, c->rv_marked_cap, (size_t)p.C * sizeof(int));
    const size_t out_bytes = (size_t)p.C * 16 + (size_t)p.N * 8;
    if (!rc) rc = grow_buffer(c, c->rv_out, c->rv_out_cap, out_bytes);
    if (rc) return rc;
    const AgentW* wts = reinterpret_cast<const AgentW*>(c->rv_tab.dev + p.off_wts);
    const RvTile* tiles = reinterpret_cast<const RvTile*>(c->rv_tab.dev + p.off_tiles);
    const int* col_of = reinterpret_cast<const int*>(c->rv_tab.dev + p.off_col);
    const int* route_of = reinterpret_cast<const int*>(c->rv_tab.dev + p.off_route);
    double* d_fam = reinterpret_cast<double*>(c->rv_out);
    long long* d_view = reinterpret_cast<long long*>(c->rv_out + (size_t)p.C * 8);
    int* d_best = reinterpret_cast<int*>(c->rv_out + (size_t)p.C * 16);
    unsigned* d_flags = reinterpret_cast<unsigned*>(c->rv_out + (size_t)p.C * 16 + (size_t)p.N * 4);
    const unsigned chunks = (unsigned)((c->rv_lmax + 255) / 256);
    const size_t lds = (size_t)p.T * 3 * Pw * 4;
    const int vpw = std::max(1, 4 / (p.T / kRvBlock));                  // view groups of a scoring workgroup (k_rv_score)
    const unsigned vchunks = (unsigned)(((c->rv_lmax + 63) / 64 + vpw - 1) / vpw);
    if (!exact) {
        rc = grow_buffer(c, c->rv_prep, c->rv_prep_cap, (size_t)p.C * 3 * Pw * 4);
        if (rc) return rc;
        const long long dwords = (long long)p.C * 3 * Pw;
        hipLaunchKernelGGL(k_rv_prep, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, c->stream, c->d_sense, (long long)p.C, P, Pw, c->rv_prep);
    }
    for (size_t k = 0; k + 1 < p.slab_tile0.size(); ++k) {
        const int s0 = (int)k * p.slab, n = std::min(p.C, s0 + p.slab) - s0;
        if (!exact) {
            const int t0 = p.slab_tile0[k], nt = p.slab_tile0[k + 1] - t0;
            hipLaunchKernelGGL(k_rv_score, dim3(vchunks, (unsigned)nt), dim3(256), lds, c->stream, c->rv_planes, c->rv_routes, tiles + t0, col_of,
                               c->rv_prep, wts, A, P, Pw, p.T, c->rv_fast, s0, p.lstride);
            hipLaunchKernelGGL(k_rv_pick<0>, dim3((unsigned)n), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, col_of, route_of, c->d_sense, wts, A,
                               P, Pw, c->rv_fast, s0, p.lstride, c->rv_delta, c->rv_marked, 0, d_fam, d_view);
        }
        // the columns whose candidates were more than the list holds (exact: every column): every view as the reference's own sum
        hipLaunchKernelGGL(k_rv_exact, dim3(chunks, (unsigned)n), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, col_of, route_of, c->d_sense, wts,
                           A, P, Pw, c->rv_marked, exact ? 1 : 0, c->rv_fast, s0, p.lstride);
        hipLaunchKernelGGL(k_rv_pick<1>, dim3((unsigned)n), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, col_of, route_of, c->d_sense, wts, A, P,
                           Pw, c->rv_fast, s0, p.lstride, c->rv_delta, c->rv_marked, exact ? 1 : 0, d_fam, d_view);
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_rv_best, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, c->stream, d_fam, err, nullptr, p.N, A, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    c->rv_out_host.resize(out_bytes);
    HIP_TRY(c, hipMemcpyAsync(c->rv_out_host.data(), c->rv_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned char* h = c->rv_out_host.data();
    std::memcpy(angle_fam, h, (size_t)p.C * 8);
    if (angle_view) std::memcpy(angle_view, h + (size_t)p.C * 8, (size_t)p.C * 8);
    std::memcpy(best_heading, h + (size_t)p.C * 16, (size_t)p.N * 4);
    if (member_flags) std::memcpy(member_flags, h + (size_t)p.C * 16 + (size_t)p.N * 4, (size_t)p.N * 4);
    return DV_OK;
}

extern "C" int dv_rviews_step_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member,
                                 const double* chem_weights, uint32_t flags, double* angle_fam, int64_t* angle_view, int32_t* best_heading) {
    const char* who = "dv_rviews_step_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !angle_fam || !best_heading) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rviews_check_tables(c, who, n_agents, n_headings, route_of_member, chem_weights);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    RvPlan p;
    rc = rviews_plan(c, p, n_agents, n_headings, route_of_member, chem_weights, nullptr);
    if (rc) return rc;
    return rviews_run(c, p, c->exact || (flags & DV_RVIEWS_EXACT), nullptr, angle_fam, angle_view, best_heading, nullptr);
}

// What the two sensed calls share: the checks, the poses, the landscape table and the patches in d_sense.
static int rviews_sense_members(dv_ctx* c, const char* who, const double* x, const double* y, const double* angles, int N, int A,
                                const int32_t* route_of_member, const double* chem_weights, const int32_t* land_of_member) {
    if (!x || !y || !angles) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rviews_check_tables(c, who, N, A, route_of_member, chem_weights);
    if (!rc) rc = rviews_check_poses(c, who, (long long)N * A);
    if (!rc) rc = sensor_fits(c, who, c->rv_h, c->rv_w);
    if (!rc) rc = land_of_member ? lands_check(c, who, "land_of_member", land_of_member, N) : noise_need_lands(c, who);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = ensure_sense_buffer(c, (size_t)N * A * c->rv_h * c->rv_w * 3);
    if (!rc && land_of_member) rc = lands_upload(c, land_of_member, N);
    if (!rc) rc = upload_member_poses(c, x, y, angles, N, A);
    if (!rc) rc = rviews_enqueue_sense(c, (long long)N * A, land_of_member ? A : 0, c->d_sense);
    return rc;
}

extern "C" int dv_rviews_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                    const int32_t* route_of_member, const double* chem_weights, const int32_t* land_of_member, uint32_t flags,
                                    double* angle_fam, int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    const char* who = "dv_rviews_sense_step";
    if (!c) return DV_ERR_INVALID;
    if (!angle_fam || !best_heading || !member_flags) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rviews_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, chem_weights, land_of_member);
    if (rc) return rc;
    RvPlan p;
    rc = rviews_plan(c, p, n_agents, n_headings, route_of_member, chem_weights, nullptr);
    if (rc) return rc;
    return rviews_run(c, p, c->exact || (flags & DV_RVIEWS_EXACT), c->rv_err, angle_fam, angle_view, best_heading, member_flags);
}

// A scene call's tables and n_out (the sum of the members' route lengths), checked before anything of the call reaches the device.
static int rviews_check_scene(dv_ctx* c, const char* who, int N, int A, const int32_t* route_of_member, const double* chem_weights, int64_t n_out) {
    int rc = rviews_check_tables(c, who, N, A, route_of_member, chem_weights);
    if (rc) return rc;
    long long total = 0;
    for (int i = 0; i < N; ++i) total += c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
    if (total != n_out) return fail(c, DV_ERR_INVALID, "%s: the members' routes hold %lld views, scene_fam %lld", who, total, (long long)n_out);
    return DV_OK;
}

// The per-view minima of the members whose patches lie in d_sense; scene_fam: the members' rows back to back, each as long as its route
// (rviews_check_scene has passed).
static int rviews_scene_run(dv_ctx* c, int N, int A, const int32_t* route_of_member, const double* chem_weights, const int* err,
                            double* scene_fam, uint32_t* member_flags) {
    std::vector<long long> row0((size_t)N);
    long long total = 0;
    for (int i = 0; i < N; ++i) {
        row0[(size_t)i] = total;
        total += c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
    }
    RvPlan p;
    int rc = rviews_plan(c, p, N, A, route_of_member, chem_weights, row0.data());
    if (!rc) rc = grow_buffer(c, c->rv_scene, c->rv_scene_cap, (size_t)total * sizeof(double));
    if (rc) return rc;
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4;
    for (int i0 = 0; i0 < N; i0 += 32768) {
        const int ni = std::min(N - i0, 32768);
        hipLaunchKernelGGL(k_rv_scene, dim3((unsigned)((c->rv_lmax + 255) / 256), (unsigned)ni), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes,
                           reinterpret_cast<const int*>(c->rv_tab.dev + p.off_route) + i0, reinterpret_cast<const long long*>(c->rv_tab.dev + p.off_row0) + i0,
                           c->d_sense + (size_t)i0 * A * P * 3, reinterpret_cast<const AgentW*>(c->rv_tab.dev + p.off_wts) + i0, A, P, Pw, c->rv_scene);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<int> herr;
    if (err) {
        herr.resize((size_t)N * A);
        HIP_TRY(c, hipMemcpyAsync(herr.data(), err, herr.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(scene_fam, c->rv_scene, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < N; ++i) {
        bool off = false;
        for (int a = 0; err && a < A; ++a) off = off || herr[(size_t)i * A + a];
        if (member_flags) member_flags[i] = off ? DV_RES_SENSE_ERROR : 0u;
        if (off) {                                                      // (the reference has reset the array to inf before it senses, :287)
            const long long len = c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
            std::fill(scene_fam + row0[(size_t)i], scene_fam + row0[(size_t)i] + len, std::numeric_limits<double>::infinity());
        }
    }
    return DV_OK;
}

extern "C" int dv_rviews_scene_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member,
                                  const double* chem_weights, int64_t n_out, double* scene_fam) {
    const char* who = "dv_rviews_scene_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !scene_fam) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rviews_check_scene(c, who, n_agents, n_headings, route_of_member, chem_weights, n_out);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rviews_scene_run(c, n_agents, n_headings, route_of_member, chem_weights, nullptr, scene_fam, nullptr);
}

extern "C" int dv_rviews_scene(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                               const int32_t* route_of_member, const double* chem_weights, const int32_t* land_of_member, int64_t n_out,
                               double* scene_fam, uint32_t* member_flags) {
    const char* who = "dv_rviews_scene";
    if (!c) return DV_ERR_INVALID;
    if (!scene_fam) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rviews_check_scene(c, who, n_agents, n_headings, route_of_member, chem_weights, n_out);
    if (!rc) rc = rviews_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, chem_weights, land_of_member);
    if (rc) return rc;
    return rviews_scene_run(c, n_agents, n_headings, route_of_member, chem_weights, c->rv_err, scene_fam, member_flags);
}
