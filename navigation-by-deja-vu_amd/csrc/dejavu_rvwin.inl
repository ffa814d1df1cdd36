// Windowed steps on the route view store (include/dejavu.h: dv_rvwin_*): perfect memory with a temporal window.  Member i is scored
// against views [win_lo[i], win_hi[i]) of ITS OWN route only, at most DV_RVWIN_MAX_VIEWS of them, and the whole of it -- integer sums,
// fast scores, candidates, the reference's sequential doubles, the first maximum -- is ONE launch whose scores never leave LDS.  The
// store, its layout, the sensing (rviews_sense_members), the patches' byte planes (k_rv_prep), the per-view sums (k_rv_score's own),
// the exact value (rv_exact_view) and the deciding launch (k_rv_best) are dejavu_rviews.inl's; nothing there changes.  The same calls with
// a threshold per member (dv_rvreloc_*, at the end of this file) add dejavu_rvreloc.inl's chain between the scoring and the deciding launch.
//
//   k_rvwin_score  workgroup = (a block of kRvBlock columns, one member).  The block's patches go to LDS as byte planes.  A wave takes
//                  64-view chunks of the member's window in turn (wave w: chunks w, w + 4, ...), a lane one view f = lo + j -- the
//                  window is not aligned to the store's groups of 64, so a wave's loads are at most two coalesced runs -- and keeps
//                  the block's two integer sums against it; the fast score of every (column, view) goes to LDS.  A window of one or two
//                  chunks would leave waves idle: its chunks are cut into 4 or 2 pixel ranges, a wave each, and the partial integer sums
//                  are added in LDS (DEJAVU_RVWIN_SPLIT=0, read at dv_create, switches the cut off for measurements).  Then wave k takes
//                  column k: the fast maximum, every view within 2 delta of it scored again as the reference's sequential double sum,
//                  the largest exact value and the least view that attains it.  Up to kRvWinCoop candidates (one, as a rule) are
//                  scored by the whole wave one after the other (rvwin_exact_wave: a lone lane's sum waits for 3 Pw dependent loads);
//                  more, a lane a candidate (rv_exact_view); more than kRvCandCap, every view of the window (at most 512) a lane each.
//                  EXACT = 1 skips the fast pass and scores every view of the window exactly.
// A column's result is a maximum and a least index over a set of views that does not depend on the order in which lanes, waves or
// workgroups run; there is no list and there are no atomics, on doubles or otherwise.
namespace dv {

constexpr int kRvWinMax = DV_RVWIN_MAX_VIEWS;  // views of a window at most: a column's fast scores are kRvWinMax doubles of LDS

constexpr int kRvWinCoop = 16;                 // candidates of a column at most that its wave scores together, one after the other

struct RvWin { int route, lo, hi, pad; };     // a member's window: views [lo, hi) of its route

// The two integer sums of kRvBlock patches (pl: their byte planes in LDS) against the view at `base`, over the dwords [q0, q1) of a
// plane: k_rv_score's sums, operation for operation.
__device__ __forceinline__ void rvwin_sums(const unsigned* __restrict__ base, const unsigned* pl, int Pw, int q0, int q1, int (&hs)[kRvBlock],
                                           int (&sv)[kRvBlock]) {
#pragma unroll
    for (int c = 0; c < kRvBlock; ++c) hs[c] = sv[c] = 0;
#pragma unroll 2
    for (int q = q0; q < q1; ++q) {
        const unsigned H = base[(long long)q * 64], S = base[(long long)(Pw + q) * 64], V = base[(long long)(2 * Pw + q) * 64];
#pragma unroll
        for (int c = 0; c < kRvBlock; ++c) {
            const unsigned ph = pl[(c * 3) * Pw + q], ps = pl[(c * 3 + 1) * Pw + q], pv = pl[(c * 3 + 2) * Pw + q];
            // the pixels whose hues differ add S_s + S_f, the others |S_s - S_f| (see k_rv_score)
            const unsigned x = ph ^ H;
            const unsigned t = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
            const unsigned one = t >> 7, ne = (t - one) | t;
            unsigned h = __builtin_amdgcn_udot4(ps, one, (unsigned)hs[c], false);
            h = __builtin_amdgcn_udot4(S, one, h, false);
            hs[c] = (int)__builtin_amdgcn_sad_u8(ps | ne, S | ne, h);
            sv[c] = (int)__builtin_amdgcn_sad_u8(pv, V, (unsigned)sv[c]);
        }
    }
}

// Lane l's value of v, for every lane (l is the wave's).
__device__ __forceinline__ double rvwin_lane(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// rv_exact_view of view f by a whole wave: 64 lanes take 64 dwords of the planes at a time and work out their 4 pixels' terms
// (rv_exact_view's, operation for operation), and the terms are added in pixel order, lane after lane, by every lane alike -- the
// reference's sequential sum, without one lane waiting for 3 * Pw dependent loads.  The value is the wave's.
__device__ __forceinline__ double rvwin_exact_wave(const unsigned* __restrict__ planes, const RvRoute& rt, long long f, const unsigned char* __restrict__ patch,
                                                   int P, int Pw, double cw, double wv, int lane) {
    const unsigned* __restrict__ base = rv_view_base(planes, rt, f, Pw);
    double diff = 0.0;
    for (int q0 = 0; q0 < Pw; q0 += 64) {
        const int q = q0 + lane;
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        if (q < Pw) {
            const unsigned H = base[(long long)q * 64], S = base[(long long)(Pw + q) * 64], V = base[(long long)(2 * Pw + q) * 64];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int px = 4 * q + k;
                if (px < P) {
                    const int hf = (int)((H >> (8 * k)) & 0xffu), sf = (int)((S >> (8 * k)) & 0xffu), vf = (int)((V >> (8 * k)) & 0xffu);
                    const int hp = patch[px * 3], sp = patch[px * 3 + 1], vp = patch[px * 3 + 2];
                    const int hsv = hp == hf ? abs(sp - sf) : sp + sf;
                    t[k] = px_term(hsv, abs(vp - vf), cw, wv);
                }
            }
        }
        const int nl = Pw - q0 < 64 ? Pw - q0 : 64;
        for (int l = 0; l < nl; ++l) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * (q0 + l) + k < P) diff += rvwin_lane(t[k], l);
        }
    }
    return (double)P - diff;
}

template <int EXACT>
__global__ void __launch_bounds__(256)
k_rvwin_score(const unsigned* __restrict__ planes, const RvRoute* __restrict__ routes, const RvWin* __restrict__ wins,
              const unsigned* __restrict__ prepped, const unsigned char* __restrict__ patches, const AgentW* __restrict__ wts, int i0, int A,
              int P, int Pw, double delta, int split, double* __restrict__ out_fam, long long* __restrict__ out_view) {
    extern __shared__ double rvw_lds[];            // EXACT = 0: sc[kRvBlock][kRvWinMax], pl[kRvBlock][3][Pw], psum[4][kRvBlock][2][64]
    const int i = i0 + (int)blockIdx.y, c0 = (int)blockIdx.x * kRvBlock;
    const int nc = A - c0 < kRvBlock ? A - c0 : kRvBlock;
    const RvWin win = wins[i];
    const RvRoute rt = routes[win.route];
    const int lo = win.lo, nwin = win.hi - win.lo;                     // (1 .. kRvWinMax: checked on the host)
    const AgentW w = wts[i];
    const int tid = (int)threadIdx.x;
    const long long kNone = 0x7fffffffffffffffll;
    double* sc = rvw_lds;
    if (!EXACT) {
        unsigned* pl = reinterpret_cast<unsigned*>(rvw_lds + kRvBlock * kRvWinMax);
        for (int t = tid; t < kRvBlock * 3 * Pw; t += 256) {
            const int k = t / (3 * Pw);
            pl[t] = k < nc ? prepped[((long long)i * A + c0 + k) * 3 * Pw + (t - k * 3 * Pw)] : 0u;
        }
        __syncthreads();
        const int lane = tid & 63, wave = tid >> 6;
        const int nch = (nwin + 63) >> 6;
        const int parts = !split ? 1 : nch == 1 ? 4 : nch == 2 ? 2 : 1;   // (the workgroup's: every thread takes the same branch below)
        int hs[kRvBlock], sv[kRvBlock];
        if (parts == 1) {
            for (int j0 = wave * 64; j0 < nwin; j0 += 256) {
                const int j = j0 + lane;
                const long long f = lo + (j < nwin ? j : nwin - 1);    // (the lanes past the window's end load its last view)
                rvwin_sums(rv_view_base(planes, rt, f, Pw), pl, Pw, 0, Pw, hs, sv);
                if (j < nwin) {
#pragma unroll
                    for (int c = 0; c < kRvBlock; ++c)
                        sc[c * kRvWinMax + j] = (double)P - (w.whs * (double)hs[c] + w.wv * (double)sv[c]) / 255.0;
                }
            }
        } else {
            // a window of one or two chunks leaves waves idle: the four waves are `parts` pixel ranges of each chunk, and the partial
            // integer sums are added in LDS -- integers, so the sum is the whole range's whatever the cut
            int* psum = reinterpret_cast<int*>(pl + kRvBlock * 3 * Pw);   // [4 waves][kRvBlock][2][64 lanes]
            const int chunk = wave / parts, part = wave % parts;
            const int j = chunk * 64 + lane;
            const long long f = lo + (j < nwin ? j : nwin - 1);
            rvwin_sums(rv_view_base(planes, rt, f, Pw), pl, Pw, (int)((long long)part * Pw / parts), (int)((long long)(part + 1) * Pw / parts), hs, sv);
#pragma unroll
            for (int c = 0; c < kRvBlock; ++c) {
                psum[((wave * kRvBlock + c) * 2) * 64 + lane] = hs[c];
                psum[((wave * kRvBlock + c) * 2 + 1) * 64 + lane] = sv[c];
            }
            __syncthreads();
            if (part == 0 && j < nwin) {
#pragma unroll
                for (int c = 0; c < kRvBlock; ++c) {
                    int h = 0, v = 0;
                    for (int p = 0; p < parts; ++p) {
                        h += psum[(((chunk * parts + p) * kRvBlock + c) * 2) * 64 + lane];
                        v += psum[(((chunk * parts + p) * kRvBlock + c) * 2 + 1) * 64 + lane];
                    }
                    sc[c * kRvWinMax + j] = (double)P - (w.whs * (double)h + w.wv * (double)v) / 255.0;
                }
            }
        }
        __syncthreads();
    }
    // The pick: wave k takes column k of the block, with no workgroup barrier from here on.
    const int lane = tid & 63, k = tid >> 6;
    if (k >= nc) return;
    const long long oc = (long long)i * A + c0 + k;
    const unsigned char* __restrict__ patch = patches + oc * P * 3;
    const double* row = sc + k * kRvWinMax;
    double v = -__builtin_inf();
    long long vj = kNone;
    int n = kRvCandCap + 1;                                            // (EXACT: every view)
    double floor_ = -__builtin_inf();
    if (!EXACT) {
        double m = -__builtin_inf();
        for (int j = lane; j < nwin; j += 64)
            if (row[j] > m) m = row[j];
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(m, o);
            if (other > m) m = other;
        }
        floor_ = m - 2.0 * delta;
        n = 0;
        for (int j0 = 0; j0 < nwin; j0 += 64)
            n += __popcll(__ballot(j0 + lane < nwin && row[j0 + lane] >= floor_));
    }
    if (n <= kRvWinCoop) {
        // few candidates (one, as a rule): the wave scores each together, in ascending view order, so `>` keeps the first maximum
        for (int j0 = 0; j0 < nwin; j0 += 64) {
            unsigned long long bal = __ballot(j0 + lane < nwin && row[j0 + lane] >= floor_);
            while (bal) {
                const int j = j0 + __builtin_ctzll(bal);
                bal &= bal - 1;
                const double e = rvwin_exact_wave(planes, rt, (long long)lo + j, patch, P, Pw, w.cw, w.wv, lane);
                if (e > v) { v = e; vj = j; }
            }
        }
    } else {
        // a lane a view: the candidates, or (more than kRvCandCap of them, and EXACT) every view of the window
        const bool every = n > kRvCandCap;
        for (int j = lane; j < nwin; j += 64)
            if (every || row[j] >= floor_) {
                const double e = rv_exact_view(rv_view_base(planes, rt, (long long)lo + j, Pw), patch, P, Pw, w.cw, w.wv);
                if (e > v) { v = e; vj = j; }                           // (a lane's views ascend: its first maximum)
            }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o);
            const long long oj = __shfl_xor(vj, o);
            if (ov > v || (ov == v && oj < vj)) { v = ov; vj = oj; }
        }
    }
    if (lane == 0) { out_fam[oc] = v; out_view[oc] = lo + vj; }
}

}  // namespace dv

static size_t rvwin_lds_bytes(int Pw, bool exact) {
    return exact ? 0 : (size_t)kRvBlock * kRvWinMax * sizeof(double) + (size_t)kRvBlock * 3 * Pw * 4 + (size_t)4 * kRvBlock * 2 * 64 * 4;
}

// The tables of a windowed call, checked entry by entry before anything of the call reaches the device.
static int rvwin_check(dv_ctx* c, const char* who, int N, int A, const int32_t* route_of_member, const double* chem_weights,
                       const int32_t* win_lo, const int32_t* win_hi) {
    int rc = rviews_check_tables(c, who, N, A, route_of_member, chem_weights);
    if (rc) return rc;
    if (!win_lo || !win_hi) return fail(c, DV_ERR_INVALID, "%s: NULL window table", who);
    for (int i = 0; i < N; ++i) {
        const long long len = c->rv_first[(size_t)route_of_member[i] + 1] - c->rv_first[(size_t)route_of_member[i]];
        const long long lo = win_lo[i], hi = win_hi[i];
        if (lo < 0 || lo >= hi || hi > len || hi - lo > DV_RVWIN_MAX_VIEWS)
            return fail(c, DV_ERR_INVALID, "%s: member %d: window [%lld, %lld) must hold 1 to %d views within its route %d of %lld views", who, i, lo,
                        hi, DV_RVWIN_MAX_VIEWS, (int)route_of_member[i], len);
    }
    return DV_OK;
}

// Score the N * A columns whose patches lie in d_sense, member i against its window; err: a word per column, or nullptr.  The call's
// tables travel in one copy to a table of their own (rvw_tab): the unwindowed calls' rv_tab, and what its mirror says of the device,
// stay as they were.  reloc_below (nullptr but in dv_rvreloc_*): the members' thresholds; the call's tables grow by dejavu_rvreloc.inl's,
// and its chain by the plan and the whole-route scoring of the lost members, between the windowed scoring and the deciding launch.
static int rvwin_run(dv_ctx* c, int N, int A, const int32_t* route_of_member, const double* chem_weights, const int32_t* win_lo,
                     const int32_t* win_hi, bool exact, const int* err, double* angle_fam, int64_t* angle_view, int32_t* best_heading,
                     uint32_t* member_flags, const double* reloc_below = nullptr) {
    const int P = c->rv_h * c->rv_w, Pw = (P + 3) / 4, C = N * A;
    const size_t off_win = (size_t)N * sizeof(AgentW);
    std::vector<unsigned char> tab(off_win + (size_t)N * sizeof(RvWin), 0);
    AgentW* w = reinterpret_cast<AgentW*>(tab.data());
    RvWin* win = reinterpret_cast<RvWin*>(tab.data() + off_win);
    for (int i = 0; i < N; ++i) {
        w[i] = AgentW{chem_weights[i], 0.5 * chem_weights[i], 1 - chem_weights[i], 0.0};   // as rviews_plan computes its own
        win[i] = RvWin{route_of_member[i], win_lo[i], win_hi[i], 0};
    }
    RvReloc reloc;
    if (reloc_below) rvreloc_tables(c, reloc, N, A, route_of_member, reloc_below, tab);
    int rc = table_upload(c, c->rvw_tab, tab.data(), tab.size());
    if (!rc && reloc_below) rc = rvreloc_buffers(c, reloc);
    const size_t out_bytes = (size_t)C * 16 + (size_t)N * 8;
    if (!rc) rc = grow_buffer(c, c->rv_out, c->rv_out_cap, out_bytes);
    if (!rc && !exact) rc = grow_buffer(c, c->rv_prep, c->rv_prep_cap, (size_t)C * 3 * Pw * 4);
    if (rc) return rc;
    const size_t lds = rvwin_lds_bytes(Pw, exact);
    if (lds > 64 * 1024 && !c->rvw_lds_opted) {                         // once per context: more than 64 KB of LDS has to be asked for
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_rvwin_score<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)rvwin_lds_bytes(kRvMaxPixels / 4, false)));
        c->rvw_lds_opted = true;
    }
    const AgentW* wts = reinterpret_cast<const AgentW*>(c->rvw_tab.dev);
    const RvWin* wins = reinterpret_cast<const RvWin*>(c->rvw_tab.dev + off_win);
    double* d_fam = reinterpret_cast<double*>(c->rv_out);
    long long* d_view = reinterpret_cast<long long*>(c->rv_out + (size_t)C * 8);
    int* d_best = reinterpret_cast<int*>(c->rv_out + (size_t)C * 16);
    unsigned* d_flags = reinterpret_cast<unsigned*>(c->rv_out + (size_t)C * 16 + (size_t)N * 4);
    if (!exact) {
        const long long dwords = (long long)C * 3 * Pw;
        hipLaunchKernelGGL(k_rv_prep, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, c->stream, c->d_sense, (long long)C, P, Pw, c->rv_prep);
    }
    const unsigned blocks = (unsigned)((A + kRvBlock - 1) / kRvBlock);
    for (int i0 = 0; i0 < N; i0 += 32768) {                             // (members are a grid's y)
        const unsigned ni = (unsigned)std::min(N - i0, 32768);
        if (exact)
            hipLaunchKernelGGL(k_rvwin_score<1>, dim3(blocks, ni), dim3(256), lds, c->stream, c->rv_planes, c->rv_routes, wins, c->rv_prep, c->d_sense,
                               wts, i0, A, P, Pw, c->rv_delta, c->rvw_split_env, d_fam, d_view);
        else
            hipLaunchKernelGGL(k_rvwin_score<0>, dim3(blocks, ni), dim3(256), lds, c->stream, c->rv_planes, c->rv_routes, wins, c->rv_prep, c->d_sense,
                               wts, i0, A, P, Pw, c->rv_delta, c->rvw_split_env, d_fam, d_view);
    }
    HIP_TRY(c, hipGetLastError());
    if (reloc_below) {
        rc = rvreloc_enqueue(c, reloc, exact, err, wts, d_fam, d_view);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_rv_best, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, d_fam, err,
                       reloc_below ? rvreloc_dev(c->rvw_plan, reloc).lost : nullptr, N, A, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    c->rv_out_host.resize(out_bytes);
    HIP_TRY(c, hipMemcpyAsync(c->rv_out_host.data(), c->rv_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned char* h = c->rv_out_host.data();
    std::memcpy(angle_fam, h, (size_t)C * 8);
    if (angle_view) std::memcpy(angle_view, h + (size_t)C * 8, (size_t)C * 8);
    std::memcpy(best_heading, h + (size_t)C * 16, (size_t)N * 4);
    if (member_flags) std::memcpy(member_flags, h + (size_t)C * 16 + (size_t)N * 4, (size_t)N * 4);
    return DV_OK;
}

extern "C" int dv_rvwin_step_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member,
                                const double* chem_weights, const int32_t* win_lo, const int32_t* win_hi, uint32_t flags, double* angle_fam,
                                int64_t* angle_view, int32_t* best_heading) {
    const char* who = "dv_rvwin_step_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !angle_fam || !best_heading) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvwin_check(c, who, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rvwin_run(c, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi, c->exact || (flags & DV_RVIEWS_EXACT), nullptr,
                     angle_fam, angle_view, best_heading, nullptr);
}

extern "C" int dv_rvwin_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                   const int32_t* route_of_member, const double* chem_weights, const int32_t* land_of_member,
                                   const int32_t* win_lo, const int32_t* win_hi, uint32_t flags, double* angle_fam, int64_t* angle_view,
                                   int32_t* best_heading, uint32_t* member_flags) {
    const char* who = "dv_rvwin_sense_step";
    if (!c) return DV_ERR_INVALID;
    if (!angle_fam || !best_heading || !member_flags) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvwin_check(c, who, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi);
    if (!rc) rc = rviews_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, chem_weights, land_of_member);
    if (rc) return rc;
    return rvwin_run(c, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi, c->exact || (flags & DV_RVIEWS_EXACT), c->rv_err,
                     angle_fam, angle_view, best_heading, member_flags);
}

// ---- the two windowed calls with a threshold per member: a lost member re-localises inside the step (dejavu_rvreloc.inl) ------------------
extern "C" int dv_rvreloc_step_u8(dv_ctx* c, const uint8_t* patches, int n_agents, int n_headings, const int32_t* route_of_member,
                                  const double* chem_weights, const int32_t* win_lo, const int32_t* win_hi, const double* reloc_below,
                                  uint32_t flags, double* angle_fam, int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    const char* who = "dv_rvreloc_step_u8";
    if (!c) return DV_ERR_INVALID;
    if (!patches || !angle_fam || !best_heading || !member_flags) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvwin_check(c, who, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi);
    if (!rc) rc = rvreloc_check(c, who, n_agents, n_headings, reloc_below);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_agents * n_headings * c->rv_h * c->rv_w * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_sense, patches, bytes, hipMemcpyHostToDevice, c->stream));
    return rvwin_run(c, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi, c->exact || (flags & DV_RVIEWS_EXACT), nullptr,
                     angle_fam, angle_view, best_heading, member_flags, reloc_below);
}

extern "C" int dv_rvreloc_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                     const int32_t* route_of_member, const double* chem_weights, const int32_t* land_of_member,
                                     const int32_t* win_lo, const int32_t* win_hi, const double* reloc_below, uint32_t flags,
                                     double* angle_fam, int64_t* angle_view, int32_t* best_heading, uint32_t* member_flags) {
    const char* who = "dv_rvreloc_sense_step";
    if (!c) return DV_ERR_INVALID;
    if (!angle_fam || !best_heading || !member_flags) return fail(c, DV_ERR_INVALID, "%s: NULL argument", who);
    int rc = rvwin_check(c, who, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi);
    if (!rc) rc = rvreloc_check(c, who, n_agents, n_headings, reloc_below);
    if (!rc) rc = rviews_sense_members(c, who, x, y, angles, n_agents, n_headings, route_of_member, chem_weights, land_of_member);
    if (rc) return rc;
    return rvwin_run(c, n_agents, n_headings, route_of_member, chem_weights, win_lo, win_hi, c->exact || (flags & DV_RVIEWS_EXACT), c->rv_err,
                     angle_fam, angle_view, best_heading, member_flags, reloc_below);
}
