// NCC on the route view store (include/dejavu.h: dv_rvncc_*): every member's headings scored by the correlation coefficient (zero-mean
// normalised cross-correlation) of ONE channel against the views of its own route.  With P pixels, a' = a - 128, b' = b - 128 and
// exact integers
//     num = P sum a'b' - sum a' sum b'      Va = P sum a'^2 - (sum a')^2      Vb = P sum b'^2 - (sum b')^2
//     q   = 0.0 if Va == 0 or Vb == 0,  else clip(double(num) / sqrt(double(Va) * double(Vb)), -1, 1)
// (none of the three changes when 128 is taken off every byte).  The cross term is dv_rvssd_*'s int8 GEMM, rvssd_group_acc
// (dejavu_rvssd.inl) unchanged; the sums are constants per view and per column; num, Va and Vb reach 2^38, so the epilogue is in
// 64-bit integers and their conversions to double are exact.  One product, one square root, one quotient, each rounded on its own
// (-ffp-contract=off): the bits are those of the same three operations on any IEEE machine.
//
//   k_rvncc_stats   sum b' and sum b'^2 per view of one channel: once per (store, channel), kept in the context until the store
//                   changes (dv_ctx::rvn_stat_gen against rv_gen), beside dv_rvssd_*'s norms and apart from them.
//   k_rvncc_prep    per route-sorted column s: k_rvssd_prep's operand row, and sum a' and sum a'^2.
//   k_rvncc_score   k_rvssd_score's grid and tiles.  A step call reduces the pairs (q, view), larger q first, then lesser view, over
//                   the 32 lanes of a half-wave by shuffles and writes ONE partial per (sorted column, view group); a wave whose group
//                   lies past its route writes the partial that loses to every other.  No memset, no atomics.  A scene call takes per
//                   (member, view) the least q over the member's headings by a 64-bit integer atomicMin on an order-preserving
//                   encoding of the double, on words of all ones: a minimum of integers does not depend on the order.  A route's
//                   padding views are masked by index (a zero view has Vb = 0 and would score 0.0, above every negative q).
//   k_rvncc_pick    a sorted column's partials reduced in view-group order -> ncc[oc], view[oc] of the caller's columns.
//   k_rvncc_best    a member's first largest column (np.argmax), its off-landscape flag.
//   k_rvncc_rows    a scene call's encoded rows as doubles, in place.
namespace dv {

// grid = ceil(n_groups * 64 / 256): thread = (group, view); sum[g * 64 + view], sq[g * 64 + view].
__global__ void __launch_bounds__(256)
k_rvncc_stats(const unsigned* __restrict__ planes, long long n_groups, int channel, int P, int Pw, int* __restrict__ sum,
              unsigned* __restrict__ sq) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_groups * 64) return;
    const unsigned* __restrict__ base = planes + ((t >> 6) * 3 + channel) * Pw * 64 + (t & 63);
    int sm = 0;
    unsigned nrm = 0;
    for (int q = 0; q < Pw; ++q) {
        const unsigned w = base[(long long)q * 64];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * q + k < P) {
                const int d = (int)((w >> (8 * k)) & 0xffu) - 128;
                sm += d;
                nrm += (unsigned)(d * d);
            }
    }
    sum[t] = sm;
    sq[t] = nrm;
}

// grid = columns, workgroup = sorted column s: op[s][Kp * 8] dwords as k_rvssd_prep lays them out, psum[s] and psq[s].
__global__ void __launch_bounds__(256)
k_rvncc_prep(const unsigned char* __restrict__ patches, const int* __restrict__ col_of, int channel, int P, int Kp, unsigned* __restrict__ op,
             int* __restrict__ psum, unsigned* __restrict__ psq) {
    __shared__ int red_s[4];
    __shared__ unsigned red_q[4];
    const long long s = blockIdx.x;
    const unsigned char* __restrict__ p = patches + (long long)col_of[s] * P * 3 + channel;
    int sm = 0;
    unsigned nrm = 0;
    for (int d = threadIdx.x; d < Kp * 8; d += 256) {
        unsigned w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * d + k < P) {
                const unsigned x = p[(long long)(4 * d + k) * 3];
                const int v = (int)x - 128;
                sm += v;
                nrm += (unsigned)(v * v);
                w |= (x ^ 0x80u) << (8 * k);
            }
        op[s * Kp * 8 + d] = w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sm += __shfl_xor(sm, o);
        nrm += __shfl_xor(nrm, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red_s[threadIdx.x >> 6] = sm;
        red_q[threadIdx.x >> 6] = nrm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        psum[s] = red_s[0] + red_s[1] + red_s[2] + red_s[3];
        psq[s] = red_q[0] + red_q[1] + red_q[2] + red_q[3];
    }
}

// The epilogue: q of one pair from its cross term, the two sums and the two variances (times P^2), all exact integers.
__device__ __forceinline__ double rvncc_value(long long P, int acc, long long sa, long long sb, long long Va, long long Vb) {
    if (Va == 0 || Vb == 0) return 0.0;                                              // a constant plane correlates with nothing
    const long long num = P * (long long)acc - sa * sb;
    const double den = sqrt((double)Va * (double)Vb);
    const double q = (double)num / den;
    return fmin(fmax(q, -1.0), 1.0);
}

// A double as a 64-bit word whose unsigned order is the doubles' (no NaN comes here), and back.
__device__ __forceinline__ unsigned long long rvncc_encode(double q) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(q);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double rvncc_decode(unsigned long long e) {
    return __longlong_as_double((long long)((e >> 63) ? e & 0x7fffffffffffffffull : ~e));
}

constexpr int kRvnccNoView = 0x7fffffff;     // the view of a partial that loses to every other (its q is -inf)

// SCENE = 0: part_q / part_v[s * G + group] take sorted column s's best (q, view) within the view group, for every group below G (the
// groups of the longest route).  SCENE = 1: rows[row0[member] + view] takes the encoded least q over the member's columns.
// grid = (ceil(G / 4), tiles).
template <int SCENE>
__global__ void __launch_bounds__(256)
k_rvncc_score(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvTile* __restrict__ tiles,
              const int* __restrict__ col_of, const unsigned* __restrict__ op, const int* __restrict__ psum, const unsigned* __restrict__ psq,
              const int* __restrict__ vsum, const unsigned* __restrict__ vsq, int channel, int A, int P, int Pw, int Kp, int G,
              double* __restrict__ part_q, int* __restrict__ part_v, const long long* __restrict__ row0,
              unsigned long long* __restrict__ rows) {
    const RvTile tile = tiles[blockIdx.y];
    const RvRoute rt = routes[tile.route];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gl = (long long)blockIdx.x * kRvssdGroupsPerBlock + wave;        // the wave's view group within the route
    if (gl * 64 >= rt.len) {
        if (!SCENE && gl < G && lane < tile.n) {                                     // no view of the route here: the losing partial
            part_q[(long long)(tile.s0 + lane) * G + gl] = -INFINITY;
            part_v[(long long)(tile.s0 + lane) * G + gl] = kRvnccNoView;
        }
        return;
    }
    const int col = lane & 31, hi = lane >> 5;
    const bool has_col = col < tile.n;
    const int srow = tile.s0 + (has_col ? col : 0);
    const uint4* __restrict__ arow = reinterpret_cast<const uint4*>(op + (long long)srow * Kp * 8) + hi;
    const unsigned* __restrict__ vb = planes + ((rt.g0 + gl) * 3 + channel) * Pw * 64 + col;
    v16i_t acc0, acc1;
    rvssd_group_acc<1>(arow, has_col, vb, hi, Pw, Kp, acc0, acc1);
    // register r of a lane is (column m = (r & 3) + 8 (r >> 2) + 4 hi, view = lane & 31) of its half
    const long long f0 = gl * 64 + col, f1 = f0 + 32;                               // the lane's two views within the route
    const bool live0 = f0 < rt.len, live1 = f1 < rt.len;
    const long long PP = P;
    const long long sb0 = vsum[(rt.g0 + gl) * 64 + col], sb1 = vsum[(rt.g0 + gl) * 64 + col + 32];
    const long long Vb0 = PP * (long long)vsq[(rt.g0 + gl) * 64 + col] - sb0 * sb0;
    const long long Vb1 = PP * (long long)vsq[(rt.g0 + gl) * 64 + col + 32] - sb1 * sb1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const bool mine = m < tile.n;                                                // (the same in the 32 lanes of a half-wave)
        const int s = tile.s0 + (mine ? m : 0);
        const long long sa = psum[s];
        const long long Va = PP * (long long)psq[s] - sa * sa;
        const double q0 = rvncc_value(PP, acc0[r], sa, sb0, Va, Vb0), q1 = rvncc_value(PP, acc1[r], sa, sb1, Va, Vb1);
        if (SCENE) {
            if (mine) {
                unsigned long long* __restrict__ row = rows + row0[col_of[s] / A];
                if (live0) atomicMin(&row[f0], rvncc_encode(q0));
                if (live1) atomicMin(&row[f1], rvncc_encode(q1));
            }
        } else {
            double q = live0 ? q0 : -INFINITY;
            int v = live0 ? (int)f0 : kRvnccNoView;
            if (live1 && q1 > q) { q = q1; v = (int)f1; }                            // (f0 < f1: a tie stays with f0)
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {                                       // over the 32 views of the half-wave
                const double oq = __shfl_xor(q, o);
                const int ov = __shfl_xor(v, o);
                if (oq > q || (oq == q && ov < v)) { q = oq; v = ov; }
            }
            if (mine && col == 0) {
                part_q[(long long)s * G + gl] = q;
                part_v[(long long)s * G + gl] = v;
            }
        }
    }
}

// Sorted column s's partials in view-group order (a later group's views are all greater: only a larger q replaces) -> the caller's
// column; grid = ceil(C / 256).
__global__ void __launch_bounds__(256)
k_rvncc_pick(const double* __restrict__ part_q, const int* __restrict__ part_v, const int* __restrict__ col_of, int C, int G,
             double* __restrict__ ncc, long long* __restrict__ view) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= C) return;
    double q = part_q[(long long)s * G];
    int v = part_v[(long long)s * G];
    for (int g = 1; g < G; ++g) {
        const double oq = part_q[(long long)s * G + g];
        if (oq > q) { q = oq; v = part_v[(long long)s * G + g]; }
    }
    ncc[col_of[s]] = q;
    view[col_of[s]] = v;
}

// A member's first largest column (np.argmax) and its flags: err is a word per column (nullptr: patches were uploaded).
__global__ void __launch_bounds__(256)
k_rvncc_best(const double* __restrict__ ncc, const int* __restrict__ err, int n, int A, int* __restrict__ best, unsigned* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int b = 0, off = 0;
    for (int a = 0; a < A; ++a) {
        if (ncc[(long long)i * A + a] > ncc[(long long)i * A + b]) b = a;
        if (err && err[(long long)i * A + a]) off = 1;
    }
    best[i] = off ? -1 : b;
    flags[i] = off ? 16u : 0u;                                                       // DV_RES_SENSE_ERROR
}

// A scene call's encoded rows as doubles, in place; grid = ceil(total / 256).
__global__ void __launch_bounds__(256)
k_rvncc_rows(unsigned long long* __restrict__ rows, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < total) reinterpret_cast<double*>(rows)[t] = rvncc_decode(rows[t]);
}

}  // namespace dv

static void rvncc_free(dv_ctx* c) {
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->rvn_stat); F(c->rvn_op); F(c->rvn_part); F(c->rvn_out); F(c->rvn_rows);
    c->rvn_stat_cap = c->rvn_op_cap = c->rvn_part_cap = c->rvn_out_cap = c->rvn_rows_cap = 0;
    c->rvn_stat_gen[0] = c->rvn_stat_gen[1] = c->rvn_stat_gen[2] = 0;
}

// Enqueue what the step and scene calls share: the channel's view statistics (if this store's are not there yet), the operand rows
// and sums of the columns whose patches lie in d_sense, and the scoring launches.  The plan is rvssd_plan's (the same tiles).
template <int SCENE>
static int rvncc_enqueue_score(dv_ctx* c, const RvssdPlan& p, int channel) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4, Kp = (P + 31) / 32;
    const long long n_groups = c->rv_bytes / ((long long)3 * Pw * 64 * 4);
    const int G = (c->rv_lmax + 63) / 64;
    int rc = grow_buffer(c, c->rvn_stat, c->rvn_stat_cap, (size_t)6 * n_groups * 64 * sizeof(unsigned));
    if (!rc) rc = grow_buffer(c, c->rvn_op, c->rvn_op_cap, (size_t)p.C * ((size_t)Kp * 32 + 2 * sizeof(unsigned)));
    if (!rc && !SCENE) rc = grow_buffer(c, c->rvn_part, c->rvn_part_cap, (size_t)p.C * G * (sizeof(double) + sizeof(int)));
    if (rc) return rc;
    int* vsum = reinterpret_cast<int*>(c->rvn_stat) + (size_t)channel * n_groups * 64;
    unsigned* vsq = c->rvn_stat + (size_t)(3 + channel) * n_groups * 64;
    if (c->rvn_stat_gen[channel] != c->rv_gen) {
        hipLaunchKernelGGL(k_rvncc_stats, dim3((unsigned)((n_groups * 64 + 255) / 256)), dim3(256), 0, c->stream, c->rv_planes, n_groups, channel, P, Pw,
                           vsum, vsq);
        HIP_TRY(c, hipGetLastError());
        c->rvn_stat_gen[channel] = c->rv_gen;
    }
    int* psum = reinterpret_cast<int*>(c->rvn_op + (size_t)p.C * Kp * 8);
    unsigned* psq = c->rvn_op + (size_t)p.C * Kp * 8 + (size_t)p.C;
    double* part_q = nullptr;                                                        // a step call's partials, a scene call's rows: the other's stay null
    int* part_v = nullptr;
    unsigned long long* rows = nullptr;
    if (SCENE) {
        rows = c->rvn_rows;
    } else {
        part_q = reinterpret_cast<double*>(c->rvn_part);
        part_v = reinterpret_cast<int*>(c->rvn_part + (size_t)p.C * G * sizeof(double));
    }
    const RvTile* tiles = reinterpret_cast<const RvTile*>(c->rvs_tab.dev + p.off_tiles);
    const int* col_of = reinterpret_cast<const int*>(c->rvs_tab.dev + p.off_col);
    const long long* row0 = reinterpret_cast<const long long*>(c->rvs_tab.dev + p.off_row0);
    hipLaunchKernelGGL(k_rvncc_prep, dim3((unsigned)p.C), dim3(256), 0, c->stream, c->d_sense, col_of, channel, P, Kp, c->rvn_op, psum, psq);
    const unsigned gchunks = (unsigned)((G + kRvssdGroupsPerBlock - 1) / kRvssdGroupsPerBlock);
    for (int t0 = 0; t0 < p.n_tiles; t0 += kRvssdTilesPerLaunch) {
        const int nt = std::min(p.n_tiles - t0, kRvssdTilesPerLaunch);
        hipLaunchKernelGGL(k_rvncc_score<SCENE>, dim3(gchunks, (unsigned)nt), dim3(256), 0, c->stream, c->rv_planes, c->rv_routes, tiles + t0, col_of,
                           c->rvn_op, psum, psq, vsum, vsq, channel, p.A, P, Pw, Kp, G, part_q, part_v, row0, rows);
    }
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// Score the C columns whose patches lie in d_sense (uint8[C][P][3], the caller's order); err: a word per column, or nullptr.
static int rvncc_run(dv_ctx* c, int N, int A, const int32_t* route_of_member, int channel, const int* err, double* angle_ncc,
                     int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    RvssdPlan p;
    int rc = rvssd_plan(c, p, N, A, route_of_member, nullptr);
    const size_t out_bytes = (size_t)p.C * 16 + (size_t)p.N * 8;
    if (!rc) rc = grow_buffer(c, c->rvn_out, c->rvn_out_cap, out_bytes);
    if (!rc) rc = rvncc_enqueue_score<0>(c, p, channel);
    if (rc) return rc;
    const int G = (c->rv_lmax + 63) / 64;
    double* d_ncc = reinterpret_cast<double*>(c->rvn_out);
    long long* d_view = reinterpret_cast<long long*>(c->rvn_out + (size_t)p.C * 8);
    int* d_best = reinterpret_cast<int*>(c->rvn_out + (size_t)p.C * 16);
    unsigned* d_flags = reinterpret_cast<unsigned*>(c->rvn_out + (size_t)p.C * 16 + (size_t)p.N * 4);
    hipLaunchKernelGGL(k_rvncc_pick, dim3((unsigned)((p.C + 255) / 256)), dim3(256), 0, c->stream, reinterpret_cast<const double*>(c->rvn_part),
                       reinterpret_cast<const int*>(c->rvn_part + (size_t)p.C * G * sizeof(double)),
                       reinterpret_cast<const int*>(c->rvs_tab.dev + p.off_col), p.C, G, d_ncc, d_view);
    hipLaunchKernelGGL(k_rvncc_best, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, c->stream, d_ncc, err, p.N, A, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    c->rv_out_host.resize(out_bytes);
    HIP_TRY(c, hipMemcpyAsync(c->rv_out_host.data(), c->rvn_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned char* h = c->rv_out_host.data();
    std::memcpy(angle_ncc, h, (size_t)p.C * 8);
    if (angle_view) std::memcpy(angle_view, h + (size_t)p.C * 8, (size_t)p.C * 8);
    std::memcpy(best_heading, h + (size_t)p.C * 16, (size_t)p.N * 4);
    if (member_flags) std::memcpy(member_flags, h + (size_t)p.C * 16 + (size_t)p.N * 4, (size_t)p.N * 4);
    return DV_OK;
}

extern "C" int dv_rvncc_step_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member, int channel,
                                double* angle_ncc, int64_t* angle_view, int32_t* best_heading) {
    const char* who = "dv_rvncc_step_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !angle_ncc || !best_heading) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssd_check_tables(c, who, n_agents, n_headings, route_of_member, channel);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rvncc_run(c, n_agents, n_headings, route_of_member, channel, nullptr, angle_ncc, angle_view, best_heading, nullptr);
}

extern "C" int dv_rvncc_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                   const int32_t* route_of_member, const int32_t* land_of_member, int channel, double* angle_ncc,
                                   int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    const char* who = "dv_rvncc_sense_step";
    if (!c) return DV_ERR_INVALID;
    if (!angle_ncc || !best_heading || !member_flags) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvssd_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, land_of_member, channel);
    if (rc) return rc;
    return rvncc_run(c, n_agents, n_headings, route_of_member, channel, c->rv_err, angle_ncc, angle_view, best_heading, member_flags);
}

static int rvncc_check_scene(dv_ctx* c, const char* who, int N, int A, const int32_t* route_of_member, int channel, int64_t n_out) {
    int rc = rvssd_check_tables(c, who, N, A, route_of_member, channel);
    if (rc) return rc;
    long long total = 0;
    for (int i = 0; i < N; ++i) total += c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
    if (total != n_out) return fail(c, DV_ERR_INVALID, "%s: the members' routes hold %lld views, scene_ncc %lld", who, total, (long long)n_out);
    return DV_OK;
}

// The per-view minima of the members whose patches lie in d_sense; scene_ncc: the members' rows back to back, each as long as its
// route (rvncc_check_scene has passed).
static int rvncc_scene_run(dv_ctx* c, int N, int A, const int32_t* route_of_member, int channel, const int* err, double* scene_ncc,
                           uint32_t* member_flags) {
    std::vector<long long> row0((size_t)N);
    long long total = 0;
    for (int i = 0; i < N; ++i) {
        row0[(size_t)i] = total;
        total += c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
    }
    RvssdPlan p;
    int rc = rvssd_plan(c, p, N, A, route_of_member, row0.data());
    if (!rc) rc = grow_buffer(c, c->rvn_rows, c->rvn_rows_cap, (size_t)total * sizeof(unsigned long long));
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->rvn_rows, 0xff, (size_t)total * sizeof(unsigned long long), c->stream));
    rc = rvncc_enqueue_score<1>(c, p, channel);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rvncc_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->rvn_rows, total);
    HIP_TRY(c, hipGetLastError());
    std::vector<int> herr;
    if (err) {
        herr.resize((size_t)N * A);
        HIP_TRY(c, hipMemcpyAsync(herr.data(), err, herr.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(scene_ncc, c->rvn_rows, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < N; ++i) {
        bool off = false;
        for (int a = 0; err && a < A; ++a) off = off || herr[(size_t)i * A + a];
        if (member_flags) member_flags[i] = off ? DV_RES_SENSE_ERROR : 0u;
        if (off) {                                                                   // (the reference's array, reset to inf)
            const long long len = c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
            std::fill(scene_ncc + row0[(size_t)i], scene_ncc + row0[(size_t)i] + len, std::numeric_limits<double>::infinity());
        }
    }
    return DV_OK;
}

extern "C" int dv_rvncc_scene_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member, int channel,
                                 int64_t n_out, double* scene_ncc) {
    const char* who = "dv_rvncc_scene_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !scene_ncc) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvncc_check_scene(c, who, n_agents, n_headings, route_of_member, channel, n_out);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rvncc_scene_run(c, n_agents, n_headings, route_of_member, channel, nullptr, scene_ncc, nullptr);
}

extern "C" int dv_rvncc_scene(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                              const int32_t* route_of_member, const int32_t* land_of_member, int channel, int64_t n_out, double* scene_ncc,
                              uint32_t* member_flags) {
    const char* who = "dv_rvncc_scene";
    if (!c) return DV_ERR_INVALID;
    if (!scene_ncc) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvncc_check_scene(c, who, n_agents, n_headings, route_of_member, channel, n_out);
    if (!rc) rc = rvssd_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, land_of_member, channel);
    if (rc) return rc;
    return rvncc_scene_run(c, n_agents, n_headings, route_of_member, channel, c->rv_err, scene_ncc, member_flags);
}
