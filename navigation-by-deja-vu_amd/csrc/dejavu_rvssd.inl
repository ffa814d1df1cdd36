// SSD on the route view store (include/dejavu.h: dv_rvssd_*): every member's headings scored as the reference's `ssds`
// (navsim/util.pyx:171-184) of ONE channel against the views of its own route, on the int8 matrix cores.  In integers
//     sum (a - b)^2 = sum a'^2 + sum b'^2 - 2 sum a' b',     a' = a - 128, b' = b - 128 in [-128, 127]
// (the expansion of k_ssd_u8_mfma, dejavu_kernels.h): the cross term is an int8 GEMM of (columns of a tile) x (views of the tile's
// route), the norms are constants per view and per column, and every score is the exact integer the reference's float64 loop
// gives (at most 255^2 * 4096 = 266 342 400 < 2^31: int32 throughout).  There is no tie window, no candidate list, no second pass.
//
// The store (dejavu_rviews.inl) is read as it lies: no second copy of the views.  Of group g the chosen channel's plane is
//     planes[((g * 3 + channel) * Pw + q) * 64 + view]  =  bytes 4q .. 4q+3 of the view (0 beyond P),
// and the B operand of K-step k (32 pixels) of the 32-view half `hf` is, in lane l, dwords q = 8k + 4(l >> 5) .. +3 of view
// 32 hf + (l & 31), each XORed with 0x80808080 (k_ssd_u8_mfma's lane map).  Dwords q >= Pw are not loaded (Pw = ceil(P / 4) is not
// a multiple of 8 in general: the next plane, or the end of the store, begins there).  A zero byte is -128 after the XOR, so the pixels
// past P are zero in the PATCH operand (their products vanish whatever the view operand holds) and in neither norm; a route's padding
// views (zero bytes) are masked by index before the minimum.
//
//   k_rvssd_norms   sum (x - 128)^2 per view of one channel: once per (store, channel), kept in the context until the store changes
//                   (dv_ctx::rv_gen, which rviews_build and rviews_free count up).
//   k_rvssd_prep    per route-sorted column s: the channel of its patch as the A operand's bytes (x ^ 0x80, 0 past P) and its norm.
//   k_rvssd_score   workgroup = (4 view groups of the tile's route, one tile of at most 32 columns of one route); a wave takes a view
//                   group: per K-step one A fragment (the tile's columns) and two MFMAs (the group's halves).  The epilogue is
//                   ssd = vnorm + pnorm - 2 acc; a step call takes per column the minimum of ssd << 32 | view by a 64-bit integer
//                   atomicMin on a word of all ones, a scene call per (member, view) the maximum over the member's headings by a
//                   32-bit integer atomicMax on a zeroed word.  A minimum (maximum) of integers does not depend on the order.
//   k_rvssd_best    a member's first least column (np.argmax(-angle_ssd)), its off-landscape flag, and the results as doubles.
//   k_rvssd_rows    a scene call's integer rows as doubles.
// The scoring kernel's body lies in device functions (rvssd_load_step, rvssd_group_acc, rvssd_value, rvssd_key_min, rvssd_score_tile)
// that the windowed calls' kernels (dejavu_rvssdw.inl) are made of as well: one statement of the arithmetic.
namespace dv {

constexpr int kRvssdTile = 32;               // columns of a tile at most: the MFMA's M
constexpr int kRvssdGroupsPerBlock = 4;      // view groups of a scoring workgroup: one per wave
constexpr int kRvssdTilesPerLaunch = 32768;  // tiles of a scoring launch at most (a grid's y)

// grid = ceil(n_groups * 64 / 256): thread = (group, view); out[g * 64 + view].
__global__ void __launch_bounds__(256)
k_rvssd_norms(const unsigned* __restrict__ planes, long long n_groups, int channel, int P, int Pw, unsigned* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_groups * 64) return;
    const unsigned* __restrict__ base = planes + ((t >> 6) * 3 + channel) * Pw * 64 + (t & 63);
    unsigned nrm = 0;
    for (int q = 0; q < Pw; ++q) {
        const unsigned w = base[(long long)q * 64];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * q + k < P) {
                const int d = (int)((w >> (8 * k)) & 0xffu) - 128;
                nrm += (unsigned)(d * d);
            }
    }
    out[t] = nrm;
}

// grid = columns, workgroup = sorted column s: op[s][Kp * 8] dwords (dword d = pixels 4d .. 4d+3 of the channel, x ^ 0x80, 0 past P)
// and pnorm[s].  col_of nullptr: the caller's own order (s is the caller's column).
__global__ void __launch_bounds__(256)
k_rvssd_prep(const unsigned char* __restrict__ patches, const int* __restrict__ col_of, int channel, int P, int Kp, unsigned* __restrict__ op,
             unsigned* __restrict__ pnorm) {
    __shared__ unsigned red[4];
    const long long s = blockIdx.x;
    const unsigned char* __restrict__ p = patches + (col_of ? (long long)col_of[s] : s) * P * 3 + channel;
    unsigned nrm = 0;
    for (int d = threadIdx.x; d < Kp * 8; d += 256) {
        unsigned w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * d + k < P) {
                const unsigned x = p[(long long)(4 * d + k) * 3];
                const int v = (int)x - 128;
                nrm += (unsigned)(v * v);
                w |= (x ^ 0x80u) << (8 * k);
            }
        op[s * Kp * 8 + d] = w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nrm += __shfl_xor(nrm, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nrm;
    __syncthreads();
    if (threadIdx.x == 0) pnorm[s] = red[0] + red[1] + red[2] + red[3];
}

// The operands of K-step k of one view group whose 8 dwords all lie in the plane: a, the lane's 16 bytes of its column's operand row
// (zeros where the column does not exist); b0 / b1, dwords 8 k + 4 hi .. + 3 of views lane & 31 and 32 + (lane & 31), XORed.
__device__ __forceinline__ void rvssd_load_step(const uint4* __restrict__ arow, bool has_col, const unsigned* __restrict__ vb, int hi, int k,
                                                v4i_t& a, v4i_t& b0, v4i_t& b1) {
    const uint4 a4 = arow[2 * k];
    a = has_col ? v4i_t{(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w} : v4i_t{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned* __restrict__ src = vb + (long long)(8 * k + 4 * hi + j) * 64;
        b0[j] = (int)(src[0] ^ 0x80808080u);
        b1[j] = (int)(src[32] ^ 0x80808080u);
    }
}

// The cross terms of one view group: acc0 / acc1 = (the 32 columns of the operand rows) x (views 0 .. 31 / 32 .. 63 of the group), over
// all Kp K-steps.  arow: the lane's column's operand row at its 16 bytes of a K-step (column lane & 31, bytes 16 hi ..; has_col: the
// column exists, else zeros); vb: the group's plane of the channel at view lane & 31.  What k_rvssd_score and k_rvssdw_score
// (dejavu_rvssdw.inl) share: the K loop, the B operand's lane map, the XOR and the last partial K-step.  AHEAD: K-steps whose loads
// are issued together before their MFMAs (1: a step at a time; a workgroup that walks its view groups one after the other, with little
// else on its CU to hide a load behind, takes more).  Integer sums: the order of the K-steps does not show.
template <int AHEAD>
__device__ __forceinline__ void rvssd_group_acc(const uint4* __restrict__ arow, bool has_col, const unsigned* __restrict__ vb, int hi, int Pw, int Kp,
                                                v16i_t& acc0, v16i_t& acc1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0;
    const int kfull = Pw / 8;                                                        // K-steps whose 8 dwords all lie in the plane
    int k = 0;
    for (; k + AHEAD <= kfull; k += AHEAD) {
        v4i_t a[AHEAD], b0[AHEAD], b1[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) rvssd_load_step(arow, has_col, vb, hi, k + u, a[u], b0[u], b1[u]);
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[u], b0[u], acc0, 0, 0, 0);  // columns x views
            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[u], b1[u], acc1, 0, 0, 0);
        }
    }
    if constexpr (AHEAD > 1) {
        for (; k < kfull; ++k) {                                                     // the full K-steps that are left
            v4i_t a, b0, b1;
            rvssd_load_step(arow, has_col, vb, hi, k, a, b0, b1);
            acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b1, acc1, 0, 0, 0);
        }
    }
    if (kfull < Kp) {                                                                // the last K-step: dwords q >= Pw are not the plane's
        const uint4 a4 = arow[2 * kfull];
        const v4i_t a = has_col ? v4i_t{(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w} : v4i_t{0, 0, 0, 0};
        v4i_t b0, b1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = 8 * kfull + 4 * hi + j;
            const unsigned* __restrict__ src = vb + (long long)(q < Pw ? q : 0) * 64;
            b0[j] = q < Pw ? (int)(src[0] ^ 0x80808080u) : 0;
            b1[j] = q < Pw ? (int)(src[32] ^ 0x80808080u) : 0;
        }
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b1, acc1, 0, 0, 0);
    }
}

// The epilogue: the exact SSD from the two norms and the cross term.
__device__ __forceinline__ int rvssd_value(int vnorm, int pnorm, int acc) { return vnorm + pnorm - 2 * acc; }

// The least ssd << 32 | view over the 32 lanes of a half-wave, each with its two views f0 and f1 (live: the view counts, else all ones);
// every lane of the half-wave gets it.
__device__ __forceinline__ unsigned long long rvssd_key_min(int ssd0, int ssd1, long long f0, long long f1, bool live0, bool live1) {
    const unsigned long long none = ~0ull;
    const unsigned long long k0 = live0 ? ((unsigned long long)(unsigned)ssd0 << 32) | (unsigned long long)f0 : none;
    const unsigned long long k1 = live1 ? ((unsigned long long)(unsigned)ssd1 << 32) | (unsigned long long)f1 : none;
    unsigned long long key = k0 < k1 ? k0 : k1;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {                                               // over the 32 views of the half-wave
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    return key;
}

// One workgroup of k_rvssd_score: 4 view groups (chunk `gchunk` of the tile's route) against one tile.  BYCOL = 0: the operand rows
// and norms lie in the tiles' column order (op[s], pnorm[s]); BYCOL = 1: in the caller's (op[col_of[s]], pnorm[col_of[s]]: the rows
// of a windowed call, dejavu_rvssdw.inl, whose plan the device wrote).
template <int SCENE, int BYCOL>
__device__ __forceinline__ void rvssd_score_tile(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvTile tile, int gchunk,
                                                 const int* __restrict__ col_of, const unsigned* __restrict__ op,
                                                 const unsigned* __restrict__ pnorm, const unsigned* __restrict__ vnorm, int channel, int A, int P,
                                                 int Pw, int Kp, unsigned long long* __restrict__ keys, const long long* __restrict__ row0,
                                                 unsigned* __restrict__ rows) {
    const RvRoute rt = routes[tile.route];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gl = (long long)gchunk * kRvssdGroupsPerBlock + wave;            // the wave's view group within the route
    if (gl * 64 >= rt.len) return;
    const int col = lane & 31, hi = lane >> 5;
    const bool has_col = col < tile.n;
    // A: column `col` of the tile, 16 bytes at pixel 32 k + 16 hi (a column past the tile's: zeros, never read back)
    const int srow = tile.s0 + (has_col ? col : 0);
    const uint4* __restrict__ arow = reinterpret_cast<const uint4*>(op + (long long)(BYCOL ? col_of[srow] : srow) * Kp * 8) + hi;
    // B: views col and 32 + col of the group, dwords 8 k + 4 hi .. + 3 of the channel's plane
    const unsigned* __restrict__ vb = planes + ((rt.g0 + gl) * 3 + channel) * Pw * 64 + col;
    v16i_t acc0, acc1;
    rvssd_group_acc<1>(arow, has_col, vb, hi, Pw, Kp, acc0, acc1);
    // register r of a lane is (column m = (r & 3) + 8 (r >> 2) + 4 hi, view = lane & 31) of its half
    const long long f0 = gl * 64 + col, f1 = f0 + 32;                               // the lane's two views within the route
    const bool live0 = f0 < rt.len, live1 = f1 < rt.len;
    const unsigned* __restrict__ vn = vnorm + (rt.g0 + gl) * 64 + col;
    const int vn0 = (int)vn[0], vn1 = (int)vn[32];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const bool mine = m < tile.n;                                                // (the same in the 32 lanes of a half-wave)
        const int s = tile.s0 + (mine ? m : 0);
        const int pn = (int)pnorm[BYCOL ? col_of[s] : s];
        const int ssd0 = rvssd_value(vn0, pn, acc0[r]), ssd1 = rvssd_value(vn1, pn, acc1[r]);
        if (SCENE) {
            if (mine) {
                unsigned* __restrict__ row = rows + row0[col_of[s] / A];
                if (live0) atomicMax(&row[f0], (unsigned)ssd0);
                if (live1) atomicMax(&row[f1], (unsigned)ssd1);
            }
        } else {
            const unsigned long long key = rvssd_key_min(ssd0, ssd1, f0, f1, live0, live1);
            if (mine && col == 0 && key != ~0ull) atomicMin(&keys[s], key);
        }
    }
}

// SCENE = 0: keys[s] takes the least ssd << 32 | view of sorted column s.  SCENE = 1: rows[row0[member] + view] takes the largest ssd
// over the member's columns.  grid = (ceil(groups of the longest route / 4), tiles).
template <int SCENE>
__global__ void __launch_bounds__(256)
k_rvssd_score(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvTile* __restrict__ tiles,
              const int* __restrict__ col_of, const unsigned* __restrict__ op, const unsigned* __restrict__ pnorm,
              const unsigned* __restrict__ vnorm, int channel, int A, int P, int Pw, int Kp, unsigned long long* __restrict__ keys,
              const long long* __restrict__ row0, unsigned* __restrict__ rows) {
    rvssd_score_tile<SCENE, 0>(planes, routes, tiles[blockIdx.y], (int)blockIdx.x, col_of, op, pnorm, vnorm, channel, A, P, Pw, Kp, keys, row0, rows);
}

// keys[s] of the sorted columns -> ssd[oc], view[oc] of the caller's columns; grid = ceil(C / 256).
__global__ void __launch_bounds__(256)
k_rvssd_unsort(const unsigned long long* __restrict__ keys, const int* __restrict__ col_of, int C, double* __restrict__ ssd,
               long long* __restrict__ view) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= C) return;
    const unsigned long long key = keys[s];
    ssd[col_of[s]] = (double)(unsigned)(key >> 32);
    view[col_of[s]] = (long long)(key & 0xffffffffull);
}

// A member's first least column (np.argmax of the negated row) and its flags: err is a word per column (nullptr: patches were uploaded),
// lost a word per member (nullptr but in a relocalising call: dejavu_rvssdw.inl).
__global__ void __launch_bounds__(256)
k_rvssd_best(const double* __restrict__ ssd, const int* __restrict__ err, const int* __restrict__ lost, int n, int A, int* __restrict__ best,
             unsigned* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int b = 0, off = 0;
    for (int a = 0; a < A; ++a) {
        if (ssd[(long long)i * A + a] < ssd[(long long)i * A + b]) b = a;
        if (err && err[(long long)i * A + a]) off = 1;
    }
    best[i] = off ? -1 : b;
    flags[i] = off ? 16u : lost && lost[i] ? 32u : 0u;                               // DV_RES_SENSE_ERROR, DV_RES_RELOCALISED
}

// A scene call's integer rows as doubles, in place behind them; grid = ceil(total / 256).
__global__ void __launch_bounds__(256)
k_rvssd_rows(const unsigned* __restrict__ rows, long long total, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < total) out[t] = (double)rows[t];
}

}  // namespace dv

static void rvssd_free(dv_ctx* c) {
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->rvs_vnorm); F(c->rvs_op); F(c->rvs_keys); F(c->rvs_out); F(c->rvs_rows); F(c->rvs_plan);
    c->rvs_vnorm_cap = c->rvs_op_cap = c->rvs_keys_cap = c->rvs_out_cap = c->rvs_rows_cap = c->rvs_plan_cap = 0;
    c->rvs_norm_gen[0] = c->rvs_norm_gen[1] = c->rvs_norm_gen[2] = 0;
    table_free(c->rvs_tab);
    table_free(c->rvsw_tab);
}

// The checks of dv_rviews_* and the channel's, before anything of the call reaches the device.
static int rvssd_check_tables(dv_ctx* c, const char* who, int N, int A, const int32_t* route_of_member, int channel) {
    if (channel < 0 || channel > 2) return fail(c, DV_ERR_INVALID, "%s: channel %d outside {0, 1, 2}", who, channel);
    if (N < 1 || A < 1) return fail(c, DV_ERR_INVALID, "%s: n_agents %d and n_headings %d must be >= 1", who, N, A);
    const std::vector<double> no_weights((size_t)N, 0.0);                            // (SSD has no chemical weight)
    return rviews_check_tables(c, who, N, A, route_of_member, no_weights.data());
}

struct RvssdPlan {
    int N, A, C, n_tiles;
    size_t off_tiles, off_row0, off_col;      // the device's tables within rvs_tab (bytes from its start)
};

// rviews_plan's order (the members sorted by route, stable) cut into tiles of at most kRvssdTile columns of one route.
static int rvssd_plan(dv_ctx* c, RvssdPlan& p, int N, int A, const int32_t* route_of_member, const long long* row0) {
    p.N = N; p.A = A; p.C = N * A;
    std::vector<int> order((size_t)N);
    for (int i = 0; i < N; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return route_of_member[a] < route_of_member[b]; });
    std::vector<int> col_of((size_t)p.C);
    for (int m = 0; m < N; ++m)
        for (int a = 0; a < A; ++a) col_of[(size_t)m * A + a] = order[(size_t)m] * A + a;
    std::vector<RvTile> tiles;
    for (int s = 0; s < p.C;) {
        const int r = route_of_member[col_of[(size_t)s] / A];
        int e = s + 1;
        while (e < p.C && e - s < kRvssdTile && route_of_member[col_of[(size_t)e] / A] == r) ++e;
        tiles.push_back(RvTile{s, e - s, r, 0});
        s = e;
    }
    p.n_tiles = (int)tiles.size();
    p.off_tiles = 0;
    p.off_row0 = p.off_tiles + tiles.size() * sizeof(RvTile);
    p.off_col = p.off_row0 + (size_t)N * sizeof(long long);
    std::vector<unsigned char> tab(p.off_col + (size_t)p.C * sizeof(int), 0);
    std::memcpy(tab.data() + p.off_tiles, tiles.data(), tiles.size() * sizeof(RvTile));
    if (row0) std::memcpy(tab.data() + p.off_row0, row0, (size_t)N * sizeof(long long));
    std::memcpy(tab.data() + p.off_col, col_of.data(), col_of.size() * sizeof(int));
    return table_upload(c, c->rvs_tab, tab.data(), tab.size());
}

// The channel's view norms of the live store, worked out (enqueued) if this store's are not there yet, and room for C operand rows
// and their norms in rvs_op.
static int rvssd_norms_and_rows(dv_ctx* c, int channel, int C, unsigned*& vnorm) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4, Kp = (P + 31) / 32;
    const long long n_groups = c->rv_bytes / ((long long)3 * Pw * 64 * 4);
    int rc = grow_buffer(c, c->rvs_vnorm, c->rvs_vnorm_cap, (size_t)3 * n_groups * 64 * sizeof(unsigned));
    if (!rc) rc = grow_buffer(c, c->rvs_op, c->rvs_op_cap, (size_t)C * ((size_t)Kp * 32 + sizeof(unsigned)));
    if (rc) return rc;
    vnorm = c->rvs_vnorm + (size_t)channel * n_groups * 64;
    if (c->rvs_norm_gen[channel] != c->rv_gen) {
        hipLaunchKernelGGL(k_rvssd_norms, dim3((unsigned)((n_groups * 64 + 255) / 256)), dim3(256), 0, c->stream, c->rv_planes, n_groups, channel, P, Pw,
                           vnorm);
        HIP_TRY(c, hipGetLastError());
        c->rvs_norm_gen[channel] = c->rv_gen;
    }
    return DV_OK;
}

// Enqueue what the step and scene calls share: the channel's view norms (if this store's are not there yet), the operand rows and
// norms of the columns whose patches lie in d_sense, and the scoring launches.
template <int SCENE>
static int rvssd_enqueue_score(dv_ctx* c, const RvssdPlan& p, int channel) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4, Kp = (P + 31) / 32;
    unsigned* vnorm = nullptr;
    const int rc = rvssd_norms_and_rows(c, channel, p.C, vnorm);
    if (rc) return rc;
    unsigned* pnorm = c->rvs_op + (size_t)p.C * Kp * 8;
    const RvTile* tiles = reinterpret_cast<const RvTile*>(c->rvs_tab.dev + p.off_tiles);
    const int* col_of = reinterpret_cast<const int*>(c->rvs_tab.dev + p.off_col);
    const long long* row0 = reinterpret_cast<const long long*>(c->rvs_tab.dev + p.off_row0);
    hipLaunchKernelGGL(k_rvssd_prep, dim3((unsigned)p.C), dim3(256), 0, c->stream, c->d_sense, col_of, channel, P, Kp, c->rvs_op, pnorm);
    const unsigned gchunks = (unsigned)(((c->rv_lmax + 63) / 64 + kRvssdGroupsPerBlock - 1) / kRvssdGroupsPerBlock);
    for (int t0 = 0; t0 < p.n_tiles; t0 += kRvssdTilesPerLaunch) {
        const int nt = std::min(p.n_tiles - t0, kRvssdTilesPerLaunch);
        hipLaunchKernelGGL(k_rvssd_score<SCENE>, dim3(gchunks, (unsigned)nt), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, tiles + t0, col_of,
                           c->rvs_op, pnorm, vnorm, channel, p.A, P, Pw, Kp, c->rvs_keys, row0, c->rvs_rows);
    }
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// Score the C columns whose patches lie in d_sense (uint8[C][P][3], the caller's order); err: a word per column, or nullptr.
static int rvssd_run(dv_ctx* c, int N, int A, const int32_t* route_of_member, int channel, const int* err, double* angle_ssd,
                     int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    RvssdPlan p;
    int rc = rvssd_plan(c, p, N, A, route_of_member, nullptr);
    const size_t out_bytes = (size_t)p.C * 16 + (size_t)p.N * 8;
    if (!rc) rc = grow_buffer(c, c->rvs_keys, c->rvs_keys_cap, (size_t)p.C * sizeof(unsigned long long));
    if (!rc) rc = grow_buffer(c, c->rvs_out, c->rvs_out_cap, out_bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->rvs_keys, 0xff, (size_t)p.C * sizeof(unsigned long long), c->stream));
    rc = rvssd_enqueue_score<0>(c, p, channel);
    if (rc) return rc;
    double* d_ssd = reinterpret_cast<double*>(c->rvs_out);
    long long* d_view = reinterpret_cast<long long*>(c->rvs_out + (size_t)p.C * 8);
    int* d_best = reinterpret_cast<int*>(c->rvs_out + (size_t)p.C * 16);
    unsigned* d_flags = reinterpret_cast<unsigned*>(c->rvs_out + (size_t)p.C * 16 + (size_t)p.N * 4);
    hipLaunchKernelGGL(k_rvssd_unsort, dim3((unsigned)((p.C + 255) / 256)), dim3(256), 0, c->stream, c->rvs_keys,
                       reinterpret_cast<const int*>(c->rvs_tab.dev + p.off_col), p.C, d_ssd, d_view);
    hipLaunchKernelGGL(k_rvssd_best, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, c->stream, d_ssd, err, nullptr, p.N, A, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    c->rv_out_host.resize(out_bytes);
    HIP_TRY(c, hipMemcpyAsync(c->rv_out_host.data(), c->rvs_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned char* h = c->rv_out_host.data();
    std::memcpy(angle_ssd, h, (size_t)p.C * 8);
    if (angle_view) std::memcpy(angle_view, h + (size_t)p.C * 8, (size_t)p.C * 8);
    std::memcpy(best_heading, h + (size_t)p.C * 16, (size_t)p.N * 4);
    if (member_flags) std::memcpy(member_flags, h + (size_t)p.C * 16 + (size_t)p.N * 4, (size_t)p.N * 4);
    return DV_OK;
}

extern "C" int dv_rvssd_step_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member, int channel,
                                double* angle_ssd, int64_t* angle_view, int32_t* best_heading) {
    const char* who = "dv_rvssd_step_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !angle_ssd || !best_heading) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssd_check_tables(c, who, n_agents, n_headings, route_of_member, channel);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rvssd_run(c, n_agents, n_headings, route_of_member, channel, nullptr, angle_ssd, angle_view, best_heading, nullptr);
}

// rviews_sense_members behind the SSD calls' own checks (it runs dv_rviews_*'s again, on a table of zero weights).
static int rvssd_sense_members(dv_ctx* c, const char* who, const double* x, const double* y, const double* angles, int N, int A,
                               const int32_t* route_of_member, const int32_t* land_of_member, int channel) {
    int rc = rvssd_check_tables(c, who, N, A, route_of_member, channel);
    if (rc) return rc;
    const std::vector<double> no_weights((size_t)N, 0.0);
    return rviews_sense_members(c, who, x, y, angles, N, A, route_of_member, no_weights.data(), land_of_member);
}

extern "C" int dv_rvssd_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                   const int32_t* route_of_member, const int32_t* land_of_member, int channel, double* angle_ssd,
                                   int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    const char* who = "dv_rvssd_sense_step";
    if (!c) return DV_ERR_INVALID;
    if (!angle_ssd || !best_heading || !member_flags) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssd_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, land_of_member, channel);
    if (rc) return rc;
    return rvssd_run(c, n_agents, n_headings, route_of_member, channel, c->rv_err, angle_ssd, angle_view, best_heading, member_flags);
}

static int rvssd_check_scene(dv_ctx* c, const char* who, int N, int A, const int32_t* route_of_member, int channel, int64_t n_out) {
    int rc = rvssd_check_tables(c, who, N, A, route_of_member, channel);
    if (rc) return rc;
    long long total = 0;
    for (int i = 0; i < N; ++i) total += c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
    if (total != n_out) return fail(c, DV_ERR_INVALID, "%s: the members' routes hold %lld views, scene_ssd %lld", who, total, (long long)n_out);
    return DV_OK;
}

// The per-view maxima of the members whose patches lie in d_sense; scene_ssd: the members' rows back to back, each as long as its
// route (rvssd_check_scene has passed).
static int rvssd_scene_run(dv_ctx* c, int N, int A, const int32_t* route_of_member, int channel, const int* err, double* scene_ssd,
                           uint32_t* member_flags) {
    std::vector<long long> row0((size_t)N);
    long long total = 0;
    for (int i = 0; i < N; ++i) {
        row0[(size_t)i] = total;
        total += c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
    }
    RvssdPlan p;
    int rc = rvssd_plan(c, p, N, A, route_of_member, row0.data());
    const size_t int_bytes = ((size_t)total * sizeof(unsigned) + 7) / 8 * 8;          // the integer rows, then the doubles
    if (!rc) rc = grow_buffer(c, c->rvs_rows, c->rvs_rows_cap, int_bytes + (size_t)total * sizeof(double));
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->rvs_rows, 0, int_bytes, c->stream));
    rc = rvssd_enqueue_score<1>(c, p, channel);
    if (rc) return rc;
    double* d_rows = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(c->rvs_rows) + int_bytes);
    hipLaunchKernelGGL(k_rvssd_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->rvs_rows, total, d_rows);
    HIP_TRY(c, hipGetLastError());
    std::vector<int> herr;
    if (err) {
        herr.resize((size_t)N * A);
        HIP_TRY(c, hipMemcpyAsync(herr.data(), err, herr.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(scene_ssd, d_rows, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < N; ++i) {
        bool off = false;
        for (int a = 0; err && a < A; ++a) off = off || herr[(size_t)i * A + a];
        if (member_flags) member_flags[i] = off ? DV_RES_SENSE_ERROR : 0u;
        if (off) {                                                                   // (-scene_ssd is the reference's array, reset to inf: :287)
            const long long len = c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
            std::fill(scene_ssd + row0[(size_t)i], scene_ssd + row0[(size_t)i] + len, -std::numeric_limits<double>::infinity());
        }
    }
    return DV_OK;
}

extern "C" int dv_rvssd_scene_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member, int channel,
                                 int64_t n_out, double* scene_ssd) {
    const char* who = "dv_rvssd_scene_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !scene_ssd) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssd_check_scene(c, who, n_agents, n_headings, route_of_member, channel, n_out);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rvssd_scene_run(c, n_agents, n_headings, route_of_member, channel, nullptr, scene_ssd, nullptr);
}

extern "C" int dv_rvssd_scene(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                              const int32_t* route_of_member, const int32_t* land_of_member, int channel, int64_t n_out, double* scene_ssd,
                              uint32_t* member_flags) {
    const char* who = "dv_rvssd_scene";
    if (!c) return DV_ERR_INVALID;
    if (!scene_ssd) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssd_check_scene(c, who, n_agents, n_headings, route_of_member, channel, n_out);
    if (!rc) rc = rvssd_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, land_of_member, channel);
    if (rc) return rc;
    return rvssd_scene_run(c, n_agents, n_headings, route_of_member, channel, c->rv_err, scene_ssd, member_flags);
}
