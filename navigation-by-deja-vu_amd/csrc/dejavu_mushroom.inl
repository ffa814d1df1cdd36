// The mushroom-body familiarity model on the device (include/dejavu.h: dv_mb_*): the circuit of Ardin, Peng, Mangan, Lagogiannis &
// Webb (2016).  A view's compared plane p (uint8, N = h * w pixels, C order) excites K Kenyon cells through a fixed random fan-in of c
// pixels each, a_k = sum_j p[conn[k][j]]; the n_active cells that come first in the order (larger a first, then lower k) fire; training
// on a view clears the one-byte output weight of every cell that fired, and a view's novelty d is the number of its firing cells whose
// weight is still 1.  Integers from pixel to score: there is nothing to round and no order of summation to fix.
//
//   k_mb<MODE>   one workgroup of 4 waves per view.  The plane is staged in LDS once.  Wave w owns the contiguous cells
//                [w * span, (w + 1) * span), span a multiple of 64, and walks them 64 at a time with lane = cell, so the connectivity
//                (uint16 [c][K]: row j holds input j of every cell) is read in consecutive words and a wave's ballot sees its cells in
//                index order.
//                pass 1     a_k from c byte gathers; one LDS atomic into the WAVE's histogram over the 255 c + 1 possible sums
//                threshold  a suffix scan over the bins of the four histograms added: t with count(a > t) < n_active <= count(a >= t),
//                           the quota q = n_active - count(a > t), and from the waves' own bins at t the rank at which each wave's
//                           cells with a == t begin -- the per-wave histograms are what spares a counting pass between the two
//                pass 2     a_k again; a cell fires when a_k > t, or a_k == t and its rank among the equals (the wave's start, the
//                           equals of its earlier trips, the ballot's lower lanes) is below q: exactly the first q in index order
//                MODE kMbTrain stores 0 to wt[k] of a firing cell (plain byte stores: every writer of a byte stores the same value,
//                whichever view's workgroup it is, so a whole route is one launch); kMbScore adds wt[k] over the firing cells;
//                kMbMask writes the fired mask and t.
//   k_mb_pose    kMbScore from a pose instead of staged bytes (an ensemble's step, dv_batch_mb_sense_step): the workgroup fills its LDS
//                plane with the compared channel of the sensor model's pixels (sense_pixel) at its column's pose, so no view goes
//                through HBM, and records in a word of its own whether a pixel left the landscape.  The body after the plane is k_mb's.
//   k_mb_decide_batch  fam[a] = (double)(-d[a]) and the first maximum over a member's headings (np.argmax), one workgroup per member
//                (an agent's own step is an ensemble of one), with the member's DV_RES_SENSE_ERROR flag
//   k_mb_count   the number of zero weights of each memory bank, one workgroup per bank
//
// Memory banks (dv_mbank_*).  wt is uint8[n_banks][K], bank b at wt + b K with no padding; n_banks is 1 after dv_mb_begin, and every
// dv_mb_* / dv_batch_mb_* call works on bank 0 through the kernels above.  k_mb_bank<kMbTrain>, k_mb_bank<kMbScore> and k_mb_pose_bank
// are k_mb and k_mb_pose with one more word read per workgroup: the view's bank, bank_of[(col0 + blockIdx.x) / per] (per = 1 in
// training: a bank per view; per = A in an ensemble's step: a bank per member), whose weights mb_view is handed instead of bank 0's.
// The connectivity, the selection and the LDS plane are the same.  Training views of many banks in one launch is safe for the reason one
// route is: every writer of a byte stores 0, and a workgroup writes inside its own bank only, so no order between views or banks
// matters and nothing is atomic.  The host checks every entry of a bank table against [0, n_banks) before a call's first launch.
//
// Landscape sets (dejavu_lands.inl).  k_mb_pose_bank_lands is k_mb_pose_bank with one more table: the column's landscape,
// land_of[(col0 + blockIdx.x) / per], whose first byte and shape mb_fill_pose is handed instead of the context's one landscape.  The
// plane still goes from the landscape to LDS; everything after it is mb_view.  k_mb_pose_bank_lands_sensors reads the column's sensor
// (pixel block, mask, level table) from the set's sensor table as well (dejavu_sensors.inl); it is launched only where a table is live.
//
// Population tables (dejavu_mbpop.inl).  A live table (c->mbp_pops > 0) gives every bank cells, wiring, quota and channel of its own:
// wt is then ragged, and the banked host paths below (mb_launch_bank, mb_batch's sensed launch, the banks' weights and counts) hand
// over to k_mbpop_*, which are mb_view on a per-bank descriptor.  The kernels of this file are launched only without a table, and
// the calls that assume this file's one wiring behind bank 0 are refused while one is live (mb_need_bank0).
//
// Bank sets (dejavu_mbset.inl).  MODE kMbSet is mb_view's fourth read-out: a firing cell adds wt_j[k] for each of the S banks of the
// workgroup's member (MbSetWts: S pointers, the same for every thread), and d receives S counts a view.  The selection is the code
// above it, unchanged; k_mbset<SRC> and k_mbset_decide are in that file.
namespace dv {

static constexpr int kMbTrain = 0, kMbScore = 1, kMbMask = 2, kMbSet = 3;
static constexpr int kMbWaves = 4;
static constexpr int kMbMaxFanIn = 16;
static constexpr int kMbSetMax = DV_MBSET_MAX_BANKS;

// kMbSet's read-out (dejavu_mbset.inl): the weights of the S banks of the workgroup's member, the same for every thread of it.
struct MbSetWts {
    const unsigned char* w[kMbSetMax];                       // (entries from S on: not read)
    int S;
};

__device__ __forceinline__ int mb_activity(const unsigned char* __restrict__ plane, const unsigned short* __restrict__ conn, int K, int c, int k) {
    // All kMbMaxFanIn index loads are issued together and then all the gathers: one global and one LDS latency per cell instead of c of
    // each.  No branch on c, which would serialise them: a row past c - 1 reads row c - 1 again (the line just fetched) and adds nothing.
    unsigned short idx[kMbMaxFanIn];
#pragma unroll
    for (int j = 0; j < kMbMaxFanIn; ++j) idx[j] = conn[(size_t)(j < c ? j : c - 1) * (size_t)K + k];
    int a = 0;
#pragma unroll
    for (int j = 0; j < kMbMaxFanIn; ++j) {
        const int v = (int)plane[idx[j]];
        a += j < c ? v : 0;
    }
    return a;
}

// One view of a launch, whatever its source: `fill(plane, tid)` puts the view's N bytes into the LDS plane (no barrier needed after
// it), then histogram, threshold, rank arithmetic and pass 2.  lds: the workgroup's dynamic LDS, [N rounded up to 4] plane bytes,
// [kMbWaves][nb] histogram words (nb = 255 c + 1), then 16 words of hand-over (kMbSet: and [kMbWaves][kMbSetMax] wave totals).
// d: [views] (kMbScore), [views][set.S] (kMbSet); fired: [views][K], thr: [views] (kMbMask; either may be nullptr).
template <int MODE, class Fill>
__device__ __forceinline__ void mb_view(unsigned* lds, Fill fill, int view, int N, const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                        unsigned char* __restrict__ wt, int* __restrict__ d, unsigned char* __restrict__ fired,
                                        int* __restrict__ thr, const MbSetWts& set = MbSetWts{}) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nb = 255 * c + 1;
    unsigned char* plane = reinterpret_cast<unsigned char*>(lds);
    unsigned* hist = lds + ((N + 3) >> 2);                   // [kMbWaves][nb]
    unsigned* hand = hist + kMbWaves * nb;                   // [0..3] the waves' totals, [4] t, [5] q, [6..9] the waves' starting ranks
    fill(plane, tid);
    for (int b = tid; b < kMbWaves * nb; b += kMbWaves * 64) hist[b] = 0u;
    __syncthreads();

    const int span = (((K + kMbWaves - 1) / kMbWaves) + 63) & ~63;
    const int k0 = wave * span;
    const int k1 = k0 + span < K ? k0 + span : K;            // (k0 >= K: the wave has no cells)
    unsigned* myhist = hist + wave * nb;
    for (int base = k0; base < k1; base += 64) {
        const int k = base + lane;
        const int a = mb_activity(plane, conn, K, c, k < k1 ? k : k1 - 1);   // (a lane past the end: a cell again, not counted)
        if (k < k1) atomicAdd(&myhist[a], 1u);
    }
    __syncthreads();

    // thread tid owns the bins [lo, hi); `above` = the cells in the bins of the threads after it
    const int bpt = (nb + kMbWaves * 64 - 1) / (kMbWaves * 64);
    const int lo = tid * bpt < nb ? tid * bpt : nb;
    const int hi = lo + bpt < nb ? lo + bpt : nb;
    unsigned mine = 0;
    for (int b = lo; b < hi; ++b) mine += hist[b] + hist[nb + b] + hist[2 * nb + b] + hist[3 * nb + b];
    unsigned suf = mine;                                      // inclusive suffix sum over the wave's lanes
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned u = __shfl_down(suf, off);
        if (lane + off < 64) suf += u;
    }
    if (lane == 0) hand[wave] = suf;
    __syncthreads();
    unsigned above = suf - mine;
    for (int w = wave + 1; w < kMbWaves; ++w) above += hand[w];
    for (int b = hi - 1; b >= lo; --b) {
        const unsigned h0 = hist[b], h1 = hist[nb + b], h2 = hist[2 * nb + b], h3 = hist[3 * nb + b];
        const unsigned cnt = h0 + h1 + h2 + h3;
        if (above < (unsigned)n_active && (unsigned)n_active <= above + cnt) {   // (one bin of one thread: 1 <= n_active <= K)
            hand[4] = (unsigned)b;
            hand[5] = (unsigned)n_active - above;
            hand[6] = 0u; hand[7] = h0; hand[8] = h0 + h1; hand[9] = h0 + h1 + h2;
        }
        above += cnt;
    }
    __syncthreads();
    const int t = (int)hand[4];
    const unsigned q = hand[5];
    unsigned rank0 = hand[6 + wave];                          // equals before this trip's cells
    int acc = 0;
    int accs[kMbSetMax] = {};                                 // kMbSet: one per bank of the set, every index a constant (registers)
    for (int base = k0; base < k1; base += 64) {
        const int k = base + lane;
        const bool in = k < k1;
        const int ak = mb_activity(plane, conn, K, c, in ? k : k1 - 1);
        const int a = in ? ak : -1;
        const bool eq = a == t;
        const unsigned long long m = __ballot(eq);
        const unsigned rank = rank0 + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        const bool fire = a > t || (eq && rank < q);
        rank0 += (unsigned)__popcll(m);
        if (MODE == kMbTrain) {
            if (fire) wt[k] = 0;
        } else if (MODE == kMbScore) {
            if (fire) acc += (int)wt[k];
        } else if (MODE == kMbSet) {
            if (fire) {
#pragma unroll
                for (int j = 0; j < kMbSetMax; ++j)
                    if (j < set.S) accs[j] += (int)set.w[j][k];   // (S is the workgroup's: no lane diverges here)
            }
        } else if (in && fired) {
            fired[(size_t)view * (size_t)K + k] = fire ? 1 : 0;
        }
    }
    if (MODE == kMbScore) {
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) hand[10 + wave] = (unsigned)acc;
        __syncthreads();
        if (tid == 0) d[view] = (int)(hand[10] + hand[11] + hand[12] + hand[13]);
    }
    if (MODE == kMbSet) {
        unsigned* tot = hand + 16;                            // [kMbWaves][kMbSetMax]
#pragma unroll
        for (int j = 0; j < kMbSetMax; ++j)
            if (j < set.S) {
                int a = accs[j];
                for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
                if (lane == 0) tot[wave * kMbSetMax + j] = (unsigned)a;
            }
        __syncthreads();
        if (tid < set.S)
            d[(size_t)view * (size_t)set.S + tid] =
                (int)(tot[tid] + tot[kMbSetMax + tid] + tot[2 * kMbSetMax + tid] + tot[3 * kMbSetMax + tid]);
    }
    if (MODE == kMbMask && thr && tid == 0) thr[view] = t;
}

// The two sources of a view's plane.  Staged bytes: view v's compared plane is src[v * view_stride + offset + j * px_stride], j < N (as
// k_im_prep).
__device__ __forceinline__ void mb_fill_staged(unsigned char* plane, int tid, const unsigned char* __restrict__ src, long long view_stride,
                                               int px_stride, int offset, int N) {
    const unsigned char* p = src + (size_t)blockIdx.x * (size_t)view_stride + offset;
    for (int j = tid; j < N; j += kMbWaves * 64) plane[j] = p[(size_t)j * px_stride];
}

// The sensor model: workgroup v senses channel `channel` of the g.sh x g.sw pixels at poses[v] into its LDS plane.  A pixel off the
// landscape contributes 0 and the selection runs all the same (every thread reaches every barrier); err[v] is written by this workgroup
// alone, 1 when any of its pixels was off, so the caller clears nothing beforehand.  NOISE (dejavu_noise.inl): the column's noise row
// and a N of its heading a within its member; pixel j draws at counter a N + j.
template <bool NOISE = false>
__device__ __forceinline__ void mb_fill_pose(unsigned char* plane, int tid, const unsigned char* __restrict__ land, const Pose* __restrict__ poses,
                                             const SensorCfg& g, const unsigned char* __restrict__ lut, int channel, int N, int* __restrict__ err,
                                             const NoiseRow* __restrict__ row = nullptr, unsigned long long a_N = 0) {
    const Pose p = poses[blockIdx.x];
    int off = 0;
    for (int j = tid; j < N; j += kMbWaves * 64) {
        unsigned H, S, V;
        if (!sense_pixel<NOISE>(land, g, p, lut, j / g.sw, j % g.sw, H, S, V, row, a_N)) { off = 1; H = S = V = 0; }
        plane[j] = (unsigned char)(channel == 0 ? H : channel == 1 ? S : V);
    }
    off = __syncthreads_or(off);
    if (tid == 0) err[blockIdx.x] = off;
}

// The weights of workgroup blockIdx.x's bank (the host has checked the table: 0 <= bank < n_banks).
__device__ __forceinline__ unsigned char* mb_bank(unsigned char* __restrict__ wt, int K, const int* __restrict__ bank_of, unsigned col0, unsigned per) {
    return wt + (size_t)bank_of[(col0 + blockIdx.x) / per] * (size_t)K;
}

template <int MODE>
__global__ __launch_bounds__(kMbWaves * 64) void k_mb(const unsigned char* __restrict__ src, long long view_stride, int px_stride, int offset, int N,
                                                      const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                      unsigned char* __restrict__ wt, int* __restrict__ d, unsigned char* __restrict__ fired,
                                                      int* __restrict__ thr) {
    extern __shared__ unsigned mb_lds[];
    mb_view<MODE>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_staged(plane, tid, src, view_stride, px_stride, offset, N); },
                  (int)blockIdx.x, N, conn, K, c, n_active, wt, d, fired, thr);
}

// kMbScore with the sensor model as the source.
__global__ __launch_bounds__(kMbWaves * 64) void k_mb_pose(const unsigned char* __restrict__ land, const Pose* __restrict__ poses, SensorCfg g,
                                                           const unsigned char* __restrict__ lut, int channel,
                                                           const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                           unsigned char* __restrict__ wt, int* __restrict__ d, int* __restrict__ err) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose(plane, tid, land, poses, g, lut, channel, N, err); },
                      (int)blockIdx.x, N, conn, K, c, n_active, wt, d, nullptr, nullptr);
}

// The banked forms (MODE kMbTrain or kMbScore): `wt` is bank 0's; src, poses, d and err begin at this launch's first column, which is
// column col0 of the call, and the bank table is the whole call's.
template <int MODE>
__global__ __launch_bounds__(kMbWaves * 64) void k_mb_bank(const unsigned char* __restrict__ src, long long view_stride, int px_stride, int offset,
                                                           int N, const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                           unsigned char* __restrict__ wt, int* __restrict__ d, const int* __restrict__ bank_of,
                                                           unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    mb_view<MODE>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_staged(plane, tid, src, view_stride, px_stride, offset, N); },
                  (int)blockIdx.x, N, conn, K, c, n_active, mb_bank(wt, K, bank_of, col0, per), d, nullptr, nullptr);
}

__global__ __launch_bounds__(kMbWaves * 64) void k_mb_pose_bank(const unsigned char* __restrict__ land, const Pose* __restrict__ poses, SensorCfg g,
                                                                const unsigned char* __restrict__ lut, int channel,
                                                                const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                                unsigned char* __restrict__ wt, int* __restrict__ d, int* __restrict__ err,
                                                                const int* __restrict__ bank_of, unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose(plane, tid, land, poses, g, lut, channel, N, err); },
                      (int)blockIdx.x, N, conn, K, c, n_active, mb_bank(wt, K, bank_of, col0, per), d, nullptr, nullptr);
}

// The member's decision from its 256 threads' own first maxima (bi < 0: the thread saw no heading) and error words.
__device__ __forceinline__ void mb_decide_member(int bv, int bi, int bad, int* __restrict__ best, unsigned* __restrict__ flags) {
    __shared__ int sv[256], si[256], sb[256];
    const int tid = (int)threadIdx.x;
    sv[tid] = bv; si[tid] = bi; sb[tid] = bad;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            const int ov = sv[tid + st], oi = si[tid + st];
            if (oi >= 0 && (si[tid] < 0 || ov > sv[tid] || (ov == sv[tid] && oi < si[tid]))) { sv[tid] = ov; si[tid] = oi; }
            sb[tid] |= sb[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        best[blockIdx.x] = sb[0] ? -1 : si[0];
        flags[blockIdx.x] = sb[0] ? kResSenseError : 0u;
    }
}

// One workgroup per member i of A columns: fam[i][a] = (double)(-d[i A + a]); best[i] = the member's first maximum (the larger value,
// the lower heading of equals, whichever thread held it).  perr (nullptr: the planes were uploaded) holds k_mb_pose's word per column:
// a member with one set gets best -1 and kResSenseError.
__global__ __launch_bounds__(256) void k_mb_decide_batch(const int* __restrict__ d, const int* __restrict__ perr, int A, double* __restrict__ fam,
                                                         int* __restrict__ best, unsigned* __restrict__ flags) {
    const int tid = (int)threadIdx.x;
    const size_t col0 = (size_t)blockIdx.x * (size_t)A;
    int bv = 0, bi = -1, bad = 0;
    for (int a = tid; a < A; a += 256) {                      // headings in rising order: a later equal does not replace
        const int v = -d[col0 + a];
        fam[col0 + a] = (double)v;
        if (bi < 0 || v > bv) { bv = v; bi = a; }
        if (perr) bad |= perr[col0 + a];
    }
    mb_decide_member(bv, bi, bad, best, flags);
}

// k_mb_pose_bank on a landscape set: the workgroup's column senses its member's own landscape (land_of_column).
__global__ __launch_bounds__(kMbWaves * 64) void k_mb_pose_bank_lands(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                                                      const int* __restrict__ land_of, const Pose* __restrict__ poses, SensorCfg g,
                                                                      const unsigned char* __restrict__ lut, int channel,
                                                                      const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                                      unsigned char* __restrict__ wt, int* __restrict__ d, int* __restrict__ err,
                                                                      const int* __restrict__ bank_of, unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    const unsigned char* land = land_of_column(lands, tab, land_of, col0 + blockIdx.x, per, g);
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose(plane, tid, land, poses, g, lut, channel, N, err); },
                      (int)blockIdx.x, N, conn, K, c, n_active, mb_bank(wt, K, bank_of, col0, per), d, nullptr, nullptr);
}

// ... and under the landscape's own sensor where the set has a sensor table (dejavu_sensors.inl): the workgroup is one column, so one
// entry, and every thread of it walks the same pixel block.
__global__ __launch_bounds__(kMbWaves * 64) void k_mb_pose_bank_lands_sensors(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                                                              const SensorEntry* __restrict__ sens, const unsigned char* __restrict__ luts,
                                                                              const int* __restrict__ land_of, const Pose* __restrict__ poses, SensorCfg g,
                                                                              int channel, const unsigned short* __restrict__ conn, int K, int c,
                                                                              int n_active, unsigned char* __restrict__ wt, int* __restrict__ d,
                                                                              int* __restrict__ err, const int* __restrict__ bank_of, unsigned col0,
                                                                              unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    const unsigned char* lut;
    const unsigned char* land = land_sensor_of_column(lands, tab, sens, luts, land_of, col0 + blockIdx.x, per, g, lut);
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose(plane, tid, land, poses, g, lut, channel, N, err); },
                      (int)blockIdx.x, N, conn, K, c, n_active, mb_bank(wt, K, bank_of, col0, per), d, nullptr, nullptr);
}

// The two forms above under noise rows (dejavu_noise.inl): the workgroup's column col0 + blockIdx.x is heading col % per of row col / per.
__global__ __launch_bounds__(kMbWaves * 64) void k_mb_pose_bank_lands_noise(const unsigned char* __restrict__ lands, const LandEntry* __restrict__ tab,
                                                                            const int* __restrict__ land_of, const NoiseRow* __restrict__ rows,
                                                                            const Pose* __restrict__ poses, SensorCfg g,
                                                                            const unsigned char* __restrict__ lut, int channel,
                                                                            const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                                            unsigned char* __restrict__ wt, int* __restrict__ d, int* __restrict__ err,
                                                                            const int* __restrict__ bank_of, unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    const unsigned col = col0 + blockIdx.x;
    const unsigned char* land = land_of_column(lands, tab, land_of, col, per, g);
    const NoiseRow* row = rows + col / per;
    const unsigned long long a_N = (unsigned long long)(col % per) * (unsigned)N;
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose<true>(plane, tid, land, poses, g, lut, channel, N, err, row, a_N); },
                      (int)blockIdx.x, N, conn, K, c, n_active, mb_bank(wt, K, bank_of, col0, per), d, nullptr, nullptr);
}

__global__ __launch_bounds__(kMbWaves * 64) void k_mb_pose_bank_lands_sensors_noise(const unsigned char* __restrict__ lands,
                                                                                    const LandEntry* __restrict__ tab,
                                                                                    const SensorEntry* __restrict__ sens,
                                                                                    const unsigned char* __restrict__ luts,
                                                                                    const int* __restrict__ land_of, const NoiseRow* __restrict__ rows,
                                                                                    const Pose* __restrict__ poses, SensorCfg g, int channel,
                                                                                    const unsigned short* __restrict__ conn, int K, int c, int n_active,
                                                                                    unsigned char* __restrict__ wt, int* __restrict__ d,
                                                                                    int* __restrict__ err, const int* __restrict__ bank_of,
                                                                                    unsigned col0, unsigned per) {
    extern __shared__ unsigned mb_lds[];
    const int N = g.sh * g.sw;
    const unsigned col = col0 + blockIdx.x;
    const unsigned char* lut;
    const unsigned char* land = land_sensor_of_column(lands, tab, sens, luts, land_of, col, per, g, lut);
    const NoiseRow* row = rows + col / per;
    const unsigned long long a_N = (unsigned long long)(col % per) * (unsigned)N;
    mb_view<kMbScore>(mb_lds, [&](unsigned char* plane, int tid) { mb_fill_pose<true>(plane, tid, land, poses, g, lut, channel, N, err, row, a_N); },
                      (int)blockIdx.x, N, conn, K, c, n_active, mb_bank(wt, K, bank_of, col0, per), d, nullptr, nullptr);
}

// zeros[b] = the zero weights of bank b = blockIdx.x (wt: [banks][K]).
__global__ __launch_bounds__(256) void k_mb_count(const unsigned char* __restrict__ wt, int K, long long* __restrict__ zeros) {
    __shared__ int red[256];
    const int tid = (int)threadIdx.x;
    wt += (size_t)blockIdx.x * (size_t)K;
    int s = 0;
    for (int k = tid; k < K; k += 256) s += wt[k] == 0 ? 1 : 0;
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) zeros[blockIdx.x] = (long long)red[0];
}

}  // namespace dv

static constexpr int kMbMaxPixels = 65536;                   // N of a view: a pixel index is a uint16 on the device
static constexpr int kMbMaxCells = 1 << 24;
static constexpr int kMbSlabViews = 8192;                    // views of one launch (one workgroup each) ...
static constexpr size_t kMbStageBytes = 64u << 20;           // ... and the bytes of uploaded planes, or of fired masks, it may stage

// Population tables (dejavu_mbpop.inl, which follows this file): a live one (c->mbp_pops > 0) gives every bank cells, wiring and
// channel of its own, and the banked calls below go through its kernels.
static void mbpop_drop(dv_ctx* c);
static hipError_t mbpop_lds_cap(int lds);
static int mbpop_launch_bank(dv_ctx* c, int mode, const unsigned char* d_src, long long view_stride, int px_stride, int by_channel, int n, int* d,
                             const int* d_bank_of, long long col0, int per);
static int mbpop_launch_pose(dv_ctx* c, bool on_lands, long long c0, int nc, int A);
static int mbpop_count(dv_ctx* c);
// Bank sets (dejavu_mbset.inl, which follows too): a member read out through several banks from one selection.
static void mbset_free(dv_ctx* c);
static hipError_t mbset_lds_cap();

static void mb_free(dv_ctx* c) {
    auto F = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
    F(c->mb_conn); F(c->mb_wt); F(c->mb_d); F(c->mb_fired); F(c->mb_zeros); F(c->mb_bd); F(c->mb_berr); F(c->mb_res.dev);
    c->mb_d_cap = c->mb_fired_cap = c->mb_bd_cap = c->mb_berr_cap = c->mb_res.cap = 0;
    table_free(c->mb_bank_of);
    mbset_free(c);
    mbpop_drop(c);
    c->mb_K = c->mb_N = c->mb_c = c->mb_active = c->mb_hh = c->mb_ww = 0;
    c->mb_banks = 1;
    c->mb_views.assign(1, 0);
}

static int mb_need(dv_ctx* c, const char* who) {
    if (!c->mb_wt) return fail(c, DV_ERR_STATE, "%s: no mushroom-body model (dv_mb_begin first)", who);
    return DV_OK;
}

// The calls that assume the begin's wiring behind bank 0 (dv_mb_*, dv_batch_mb_*): refused while a population table is live.
static int mb_need_bank0(dv_ctx* c, const char* who) {
    int rc = mb_need(c, who);
    if (rc) return rc;
    if (c->mbp_pops)
        return fail(c, DV_ERR_STATE, "%s: a population table is live, and bank 0 is no longer the model dv_mb_begin made (dv_mbpop_clear first, or the dv_mbank_ call)", who);
    return DV_OK;
}

static size_t mb_lds_bytes(int N, int fan_in) {
    return (size_t)((N + 3) & ~3) + (size_t)kMbWaves * (size_t)(255 * fan_in + 1) * 4u + 16u * 4u;
}
static size_t mb_lds_bytes(const dv_ctx* c) { return mb_lds_bytes(c->mb_N, c->mb_c); }

// Views of one launch when each brings `bytes_per_view` of staged bytes.
static int64_t mb_slab(size_t bytes_per_view) {
    int64_t s = (int64_t)(kMbStageBytes / (bytes_per_view ? bytes_per_view : 1));
    if (s > kMbSlabViews) s = kMbSlabViews;
    return s < 1 ? 1 : s;
}

// Enqueue one launch over n <= kMbSlabViews views resident on the device (layout as k_mb's src).
template <int MODE>
static int mb_launch(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, int offset, int n, int* d, unsigned char* fired,
                     int* thr) {
    hipLaunchKernelGGL((k_mb<MODE>), dim3((unsigned)n), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, d_src, view_stride, px_stride, offset, c->mb_N,
                       c->mb_conn, c->mb_K, c->mb_c, c->mb_active, c->mb_wt, d, fired, thr);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// The banked launch: its view v works through bank d_bank_of[(col0 + v) / per].  Training hands the table in from the launch's own
// first view on (col0 = 0, per = 1: a bank per view); an ensemble's step hands in the whole table, the launch's first column and A.
template <int MODE>
static int mb_launch_bank(dv_ctx* c, const unsigned char* d_src, long long view_stride, int px_stride, int offset, int n, int* d, const int* d_bank_of,
                          long long col0, int per) {
    // (under a population table a strided source is the sensed views, read at the bank's own channel instead of `offset`)
    if (c->mbp_pops) return mbpop_launch_bank(c, MODE, d_src, view_stride, px_stride, px_stride == 3, n, d, d_bank_of, col0, per);
    hipLaunchKernelGGL((k_mb_bank<MODE>), dim3((unsigned)n), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, d_src, view_stride, px_stride, offset,
                       c->mb_N, c->mb_conn, c->mb_K, c->mb_c, c->mb_active, c->mb_wt, d, d_bank_of, (unsigned)col0, (unsigned)per);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

// n views were trained: all into bank 0 (bank_of == nullptr), or view v into bank_of[v].
static void mb_count_views(dv_ctx* c, int64_t n, const int32_t* bank_of) {
    if (!bank_of) c->mb_views[0] += n;
    else for (int64_t v = 0; v < n; ++v) c->mb_views[(size_t)bank_of[v]] += 1;
}

// A banked call's table, checked entry by entry before anything of the call reaches the device ...
static int mbank_check(dv_ctx* c, const char* who, const char* what, const int32_t* bank_of, int64_t n) {
    return index_check(c, who, what, bank_of, n, c->mb_banks, "n_banks");
}

// ... and then enqueued for the device, unless the device's table holds the same already.
static int mbank_upload(dv_ctx* c, const int32_t* bank_of, int64_t n) {
    return table_upload(c, c->mb_bank_of, bank_of, (size_t)n * sizeof(int));
}

extern "C" int dv_mb_end(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    mb_free(c);
    return DV_OK;
}

extern "C" int dv_mb_begin(dv_ctx* c, int h, int w, int channel, int n_kc, int fan_in, int n_active, const int32_t* conn) {
    if (!c) return DV_ERR_INVALID;
    if (!conn) return fail(c, DV_ERR_INVALID, "dv_mb_begin: the connectivity is NULL");
    if (h < 1 || w < 1 || (long long)h * w > kMbMaxPixels) return fail(c, DV_ERR_INVALID, "dv_mb_begin: views of %d x %d (1..%d pixels)", h, w, kMbMaxPixels);
    if (channel < 0 || channel > 2) return fail(c, DV_ERR_INVALID, "dv_mb_begin: channel %d outside [0, 2]", channel);
    if (n_kc < 1 || n_kc > kMbMaxCells) return fail(c, DV_ERR_INVALID, "dv_mb_begin: n_kc %d outside [1, %d]", n_kc, kMbMaxCells);
    if (fan_in < 1 || fan_in > dv::kMbMaxFanIn) return fail(c, DV_ERR_INVALID, "dv_mb_begin: fan_in %d outside [1, %d]", fan_in, dv::kMbMaxFanIn);
    if (n_active < 1 || n_active > n_kc) return fail(c, DV_ERR_INVALID, "dv_mb_begin: n_active %d outside [1, n_kc = %d]", n_active, n_kc);
    const int N = h * w;
    const size_t K = (size_t)n_kc, cc = (size_t)fan_in;
    // the device's layout: uint16 [fan_in][n_kc], so that a wave's lanes read consecutive cells
    std::vector<unsigned short> ct(K * cc);
    for (size_t k = 0; k < K; ++k)
        for (size_t j = 0; j < cc; ++j) {
            const int32_t v = conn[k * cc + j];
            if (v < 0 || v >= N) return fail(c, DV_ERR_INVALID, "dv_mb_begin: conn[%zu][%zu] = %d outside [0, %d)", k, j, (int)v, N);
            ct[j * K + k] = (unsigned short)v;
        }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    mb_free(c);
    c->mb_K = n_kc; c->mb_N = N; c->mb_c = fan_in; c->mb_active = n_active; c->mb_hh = h; c->mb_ww = w; c->mb_channel = channel;
    // The cap on dynamic LDS belongs to the FUNCTION, not to this context: set to this model's own bytes, the begin of a small model in
    // one context would lower it under the launches of a larger model in another.  So it is the most any model can ask for, whatever
    // this one needs: 65536 + 4 * 4081 * 4 + 64 = 130896 of the workgroup's 160 KB.  A cap, not an allocation: a launch still takes
    // mb_lds_bytes(c) of its own model.
    const int lds = (int)mb_lds_bytes(kMbMaxPixels, dv::kMbMaxFanIn);
    hipError_t e = hipMalloc((void**)&c->mb_conn, ct.size() * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMalloc((void**)&c->mb_wt, K);
    if (e == hipSuccess) e = hipMalloc((void**)&c->mb_zeros, sizeof(long long));
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb<kMbTrain>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb<kMbScore>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb<kMbMask>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_pose, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_bank<kMbTrain>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_bank<kMbScore>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_pose_bank, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_pose_bank_lands, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_pose_bank_lands_sensors, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_pose_bank_lands_noise, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_mb_pose_bank_lands_sensors_noise, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = mbpop_lds_cap(lds);
    if (e == hipSuccess) e = mbset_lds_cap();
    if (e == hipSuccess) e = hipMemcpyAsync(c->mb_conn, ct.data(), ct.size() * sizeof(unsigned short), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->mb_wt, 1, K, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // `ct` is this call's
    if (e != hipSuccess) {
        (void)hipGetLastError();
        mb_free(c);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_mb_begin: %d cells x %d inputs: %s", n_kc, fan_in, hipGetErrorString(e));
    }
    return DV_OK;
}

// Train on n uploaded planes; bank_of == nullptr: all into bank 0 (dv_mb_train_u8), else view v into bank bank_of[v].
static int mb_train_u8(dv_ctx* c, const char* who, const uint8_t* planes, int64_t n, const int32_t* bank_of) {
    int rc = mb_need(c, who);
    if (rc) return rc;
    if (!planes || n < 0) return fail(c, DV_ERR_INVALID, "%s: planes is NULL or n < 0", who);
    if (bank_of) { rc = mbank_check(c, who, "bank_of_view", bank_of, n); if (rc) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (bank_of) { rc = mbank_upload(c, bank_of, n); if (rc) return rc; }
    const size_t N = (size_t)c->mb_N;
    int64_t slab = mb_slab(N);
    if (slab > n) slab = n;
    if (n > 0) { rc = ensure_sense_buffer(c, (size_t)slab * N); if (rc) return rc; }
    for (int64_t v0 = 0; v0 < n; v0 += slab) {
        const int64_t ns = n - v0 < slab ? n - v0 : slab;
        HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)v0 * N, (size_t)ns * N, hipMemcpyHostToDevice, c->stream));
        rc = bank_of ? mb_launch_bank<kMbTrain>(c, c->d_sense, (long long)N, 1, 0, (int)ns, nullptr, c->mb_bank_of.device<int>() + v0, 0, 1)
                     : mb_launch<kMbTrain>(c, c->d_sense, (long long)N, 1, 0, (int)ns, nullptr, nullptr, nullptr);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // the slab is reused, `planes` is borrowed
    }
    mb_count_views(c, n, bank_of);
    return DV_OK;
}

extern "C" int dv_mb_train_u8(dv_ctx* c, const uint8_t* planes, int64_t n) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_mb_train_u8");
    if (rc) return rc;
    return mb_train_u8(c, "dv_mb_train_u8", planes, n, nullptr);
}

// Sense n poses and train on their compared plane; bank_of as mb_train_u8's.  land_of == nullptr: the poses are on the context's one
// landscape (k_sense); else pose v is on landscape land_of[v] of the set (k_sense_lands).
static int mb_train_from_poses(dv_ctx* c, const char* who, const double* x, const double* y, const double* angle, int64_t n, const int32_t* bank_of,
                               const int32_t* land_of, uint8_t* out_views) {
    int rc = mb_need(c, who);
    if (rc) return rc;
    if (!x || !y || !angle || n < 1 || n > 0x7fffffff) return fail(c, DV_ERR_INVALID, "%s: bad arguments", who);
    rc = sensor_fits(c, who, c->mb_hh, c->mb_ww);
    if (rc) return rc;
    if (bank_of) { rc = mbank_check(c, who, "bank_of_view", bank_of, n); if (rc) return rc; }
    if (land_of) { rc = lands_check(c, who, "land_of_view", land_of, n); if (rc) return rc; }
    else { rc = noise_need_lands(c, who); if (rc) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (bank_of) { rc = mbank_upload(c, bank_of, n); if (rc) return rc; }
    if (land_of) { rc = lands_upload(c, land_of, n); if (rc) return rc; }
    const size_t bytes = (size_t)n * (size_t)c->mb_N * 3;
    rc = ensure_sense_buffer(c, bytes);
    if (rc) return rc;
    rc = land_of ? lands_enqueue_sense(c, x, y, angle, n) : enqueue_sense(c, x, y, angle, n, c->d_sense);
    if (rc) return rc;
    if (out_views) HIP_TRY(c, hipMemcpyAsync(out_views, c->d_sense, bytes, hipMemcpyDeviceToHost, c->stream));
    rc = land_of ? lands_check_sense_error(c, who, n) : check_sense_error(c);   // (synchronises: nothing is trained from a footprint off the landscape)
    if (rc) return rc;
    const long long stride = 3ll * c->mb_N;
    for (int64_t v0 = 0; v0 < n; v0 += kMbSlabViews) {
        const int64_t ns = n - v0 < kMbSlabViews ? n - v0 : kMbSlabViews;
        const unsigned char* src = c->d_sense + (size_t)v0 * (size_t)stride;
        rc = bank_of ? mb_launch_bank<kMbTrain>(c, src, stride, 3, c->mb_channel, (int)ns, nullptr, c->mb_bank_of.device<int>() + v0, 0, 1)
                     : mb_launch<kMbTrain>(c, src, stride, 3, c->mb_channel, (int)ns, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    mb_count_views(c, n, bank_of);
    return DV_OK;
}

extern "C" int dv_mb_train_from_poses(dv_ctx* c, const double* x, const double* y, const double* angle, int64_t n, uint8_t* out_views) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_mb_train_from_poses");
    if (rc) return rc;
    return mb_train_from_poses(c, "dv_mb_train_from_poses", x, y, angle, n, nullptr, nullptr, out_views);
}

extern "C" int dv_mb_score_u8(dv_ctx* c, const uint8_t* planes, int n, double* familiarity) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_mb_score_u8");
    if (rc) return rc;
    if (!planes || !familiarity || n < 1) return fail(c, DV_ERR_INVALID, "dv_mb_score_u8: NULL argument or n < 1");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->mb_N;
    int64_t slab = mb_slab(N);
    if (slab > n) slab = n;
    rc = ensure_sense_buffer(c, (size_t)slab * N);
    if (!rc) rc = grow_buffer(c, c->mb_d, c->mb_d_cap, (size_t)slab * sizeof(int));
    if (rc) return rc;
    std::vector<int> dh((size_t)slab);
    for (int64_t v0 = 0; v0 < n; v0 += slab) {
        const int64_t ns = n - v0 < slab ? n - v0 : slab;
        HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)v0 * N, (size_t)ns * N, hipMemcpyHostToDevice, c->stream));
        rc = mb_launch<kMbScore>(c, c->d_sense, (long long)N, 1, 0, (int)ns, c->mb_d, nullptr, nullptr);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(dh.data(), c->mb_d, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int64_t a = 0; a < ns; ++a) familiarity[v0 + a] = (double)(-dh[(size_t)a]);   // (the integer is negated: a trained view gives +0.0)
    }
    return DV_OK;
}

extern "C" int dv_mb_activity_u8(dv_ctx* c, const uint8_t* planes, int n, uint8_t* fired, int32_t* threshold) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_mb_activity_u8");
    if (rc) return rc;
    if (!planes || n < 1) return fail(c, DV_ERR_INVALID, "dv_mb_activity_u8: planes is NULL or n < 1");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->mb_N, K = (size_t)c->mb_K;
    int64_t slab = mb_slab(N > K ? N : K);
    if (slab > n) slab = n;
    rc = ensure_sense_buffer(c, (size_t)slab * N);
    if (!rc) rc = grow_buffer(c, c->mb_d, c->mb_d_cap, (size_t)slab * sizeof(int));
    if (!rc && fired) rc = grow_buffer(c, c->mb_fired, c->mb_fired_cap, (size_t)slab * K);
    if (rc) return rc;
    for (int64_t v0 = 0; v0 < n; v0 += slab) {
        const int64_t ns = n - v0 < slab ? n - v0 : slab;
        HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)v0 * N, (size_t)ns * N, hipMemcpyHostToDevice, c->stream));
        rc = mb_launch<kMbMask>(c, c->d_sense, (long long)N, 1, 0, (int)ns, nullptr, fired ? c->mb_fired : nullptr, c->mb_d);
        if (rc) return rc;
        if (fired) HIP_TRY(c, hipMemcpyAsync(fired + (size_t)v0 * K, c->mb_fired, (size_t)ns * K, hipMemcpyDeviceToHost, c->stream));
        if (threshold) HIP_TRY(c, hipMemcpyAsync(threshold + v0, c->mb_d, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return DV_OK;
}

extern "C" int dv_mb_sense_step(dv_ctx* c, double x, double y, const double* angles, int n, double* angle_fam, int32_t* best_heading) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_mb_sense_step");
    if (rc) return rc;
    if (!angles || !angle_fam || !best_heading || n < 1) return fail(c, DV_ERR_INVALID, "dv_mb_sense_step: NULL argument or n_headings < 1");
    rc = sensor_fits(c, "dv_mb_sense_step", c->mb_hh, c->mb_ww);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    double* d_fam = nullptr; int* d_best = nullptr; unsigned* d_flags = nullptr;   // the packed results' parts on the device
    rc = ensure_sense_buffer(c, (size_t)n * (size_t)c->mb_N * 3);
    if (!rc) rc = grow_buffer(c, c->mb_d, c->mb_d_cap, (size_t)n * sizeof(int));
    if (!rc) rc = packed_device(c, c->mb_res, n, 1, d_fam, d_best, d_flags);
    if (rc) return rc;
    c->mb_xy.assign((size_t)n, x);
    c->mb_xy.resize(2 * (size_t)n, y);
    rc = enqueue_sense(c, c->mb_xy.data(), c->mb_xy.data() + n, angles, n, c->d_sense);
    if (rc) return rc;
    const long long stride = 3ll * c->mb_N;
    for (int v0 = 0; v0 < n; v0 += kMbSlabViews) {            // every heading in one launch (a launch's grid: kMbSlabViews workgroups)
        const int ns = n - v0 < kMbSlabViews ? n - v0 : kMbSlabViews;
        rc = mb_launch<kMbScore>(c, c->d_sense + (size_t)v0 * (size_t)stride, stride, 3, c->mb_channel, ns, c->mb_d + v0, nullptr, nullptr);
        if (rc) return rc;
    }
    // an ensemble of one whose patches are in d_sense: no word per pose (k_sense's one flag is read below), so the member's flag is 0
    hipLaunchKernelGGL(k_mb_decide_batch, dim3(1), dim3(256), 0, c->stream, c->mb_d, (const int*)nullptr, n, d_fam, d_best, d_flags);
    HIP_TRY(c, hipGetLastError());
    rc = packed_fetch(c, c->mb_res, n, 1);
    if (!rc) rc = check_sense_error(c);                       // (synchronises; a footprint off the landscape: DV_ERR_INDEX)
    if (rc) return rc;
    packed_unpack(c->mb_res, n, 1, angle_fam, best_heading, nullptr);
    return DV_OK;
}

// ---- ensembles: every member's headings in one enqueue and one wait ----------------------------------------------------------
// planes != nullptr: uploaded uint8[n_agents][A][h][w], scored by k_mb<kMbScore> in launches of mb_slab(N) columns (the view bound and
// the byte bound of dv_mb_score_u8); else the poses (x[i], y[i], angles[i][a]) go to k_mb_pose, kMbSlabViews columns a launch.  The
// launches follow one another on the stream; the host waits once, for the one copy of the packed results.
// bank_of == nullptr: every member scores under bank 0 (the dv_batch_mb_* calls); else member i under bank bank_of[i], through the
// banked kernels -- the same enqueue, with the members' table uploaded ahead of the launches.
// land_of != nullptr (poses and banks only): member i senses landscape land_of[i] of the set, through k_mb_pose_bank_lands, or through
// k_mb_pose_bank_lands_sensors under that landscape's own sensor where the set has a sensor table.
static int mb_batch(dv_ctx* c, const char* who, const uint8_t* planes, const double* x, const double* y, const double* angles, int n_agents, int A,
                    const int32_t* bank_of, const int32_t* land_of, double* angle_fam, int32_t* best_heading, uint32_t* flags) {
    const long long C = (long long)n_agents * A;
    if (C > 0x7fffffffll) return fail(c, DV_ERR_INVALID, "%s: %d agents x %d headings are too many columns", who, n_agents, A);
    if (bank_of) { const int rb = mbank_check(c, who, "bank_of_member", bank_of, n_agents); if (rb) return rb; }
    if (land_of) { const int rl = lands_check(c, who, "land_of_member", land_of, n_agents); if (rl) return rl; }
    else if (!planes) { const int rl = noise_need_lands(c, who); if (rl) return rl; }
    if (!planes && c->nz_n && c->mbp_pops)                      // (the population table's pose kernels have no noise form)
        return fail(c, DV_ERR_STATE, "%s: noise rows are live, and the sensed step under a population table has no noise form (dv_noise_clear first)", who);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->mb_N;
    long long slab = planes ? (long long)mb_slab(N) : (long long)kMbSlabViews;
    if (slab > C) slab = C;
    double* d_fam = nullptr; int* d_best = nullptr; unsigned* d_flags = nullptr;   // the packed results' parts on the device
    int rc = grow_buffer(c, c->mb_bd, c->mb_bd_cap, (size_t)C * sizeof(int));
    if (!rc) rc = packed_device(c, c->mb_res, C, n_agents, d_fam, d_best, d_flags);
    if (!rc && !planes) rc = grow_buffer(c, c->mb_berr, c->mb_berr_cap, (size_t)C * sizeof(int));
    if (!rc && planes) rc = ensure_sense_buffer(c, (size_t)slab * N);
    if (!rc && bank_of) rc = mbank_upload(c, bank_of, n_agents);
    if (!rc && land_of) rc = lands_upload(c, land_of, n_agents);
    if (rc) return rc;
    if (!planes) {
        rc = upload_member_poses(c, x, y, angles, n_agents, A);
        if (rc) return rc;
    }
    for (long long c0 = 0; c0 < C; c0 += slab) {
        const int nc = (int)(C - c0 < slab ? C - c0 : slab);
        if (planes) {
            HIP_TRY(c, hipMemcpyAsync(c->d_sense, planes + (size_t)c0 * N, (size_t)nc * N, hipMemcpyHostToDevice, c->stream));
            rc = bank_of ? mb_launch_bank<kMbScore>(c, c->d_sense, (long long)N, 1, 0, nc, c->mb_bd + c0, c->mb_bank_of.device<int>(), c0, A)
                         : mb_launch<kMbScore>(c, c->d_sense, (long long)N, 1, 0, nc, c->mb_bd + c0, nullptr, nullptr);
            if (rc) return rc;
        } else if (c->mbp_pops) {                               // (bank_of is there: the bank-0 calls are refused under a table)
            rc = mbpop_launch_pose(c, land_of != nullptr, c0, nc, A);
            if (rc) return rc;
        } else if (land_of && c->nz_n && c->sn_tab) {             // (noise rows: uploaded beside the landscape table, dejavu_noise.inl)
            hipLaunchKernelGGL(k_mb_pose_bank_lands_sensors_noise, dim3((unsigned)nc), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, c->ld_lands,
                               c->ld_tab, c->sn_tab, c->sn_luts, c->ld_of.device<int>(), c->nz_tab.device<NoiseRow>(), c->d_poses + c0, c->sensor,
                               c->mb_channel, c->mb_conn, c->mb_K, c->mb_c, c->mb_active, c->mb_wt, c->mb_bd + c0, c->mb_berr + c0,
                               c->mb_bank_of.device<int>(), (unsigned)c0, (unsigned)A);
            HIP_TRY(c, hipGetLastError());
        } else if (land_of && c->nz_n) {
            hipLaunchKernelGGL(k_mb_pose_bank_lands_noise, dim3((unsigned)nc), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, c->ld_lands, c->ld_tab,
                               c->ld_of.device<int>(), c->nz_tab.device<NoiseRow>(), c->d_poses + c0, c->sensor, c->d_lut, c->mb_channel, c->mb_conn,
                               c->mb_K, c->mb_c, c->mb_active, c->mb_wt, c->mb_bd + c0, c->mb_berr + c0, c->mb_bank_of.device<int>(), (unsigned)c0,
                               (unsigned)A);
            HIP_TRY(c, hipGetLastError());
        } else if (land_of && c->sn_tab) {
            hipLaunchKernelGGL(k_mb_pose_bank_lands_sensors, dim3((unsigned)nc), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, c->ld_lands, c->ld_tab,
                               c->sn_tab, c->sn_luts, c->ld_of.device<int>(), c->d_poses + c0, c->sensor, c->mb_channel, c->mb_conn, c->mb_K, c->mb_c,
                               c->mb_active, c->mb_wt, c->mb_bd + c0, c->mb_berr + c0, c->mb_bank_of.device<int>(), (unsigned)c0, (unsigned)A);
            HIP_TRY(c, hipGetLastError());
        } else if (land_of) {
            hipLaunchKernelGGL(k_mb_pose_bank_lands, dim3((unsigned)nc), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, c->ld_lands, c->ld_tab,
                               c->ld_of.device<int>(), c->d_poses + c0, c->sensor, c->d_lut, c->mb_channel, c->mb_conn, c->mb_K, c->mb_c, c->mb_active,
                               c->mb_wt, c->mb_bd + c0, c->mb_berr + c0, c->mb_bank_of.device<int>(), (unsigned)c0, (unsigned)A);
            HIP_TRY(c, hipGetLastError());
        } else if (bank_of) {
            hipLaunchKernelGGL(k_mb_pose_bank, dim3((unsigned)nc), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, c->d_land, c->d_poses + c0, c->sensor,
                               c->d_lut, c->mb_channel, c->mb_conn, c->mb_K, c->mb_c, c->mb_active, c->mb_wt, c->mb_bd + c0, c->mb_berr + c0,
                               c->mb_bank_of.device<int>(), (unsigned)c0, (unsigned)A);
            HIP_TRY(c, hipGetLastError());
        } else {
            hipLaunchKernelGGL(k_mb_pose, dim3((unsigned)nc), dim3(kMbWaves * 64), mb_lds_bytes(c), c->stream, c->d_land, c->d_poses + c0, c->sensor,
                               c->d_lut, c->mb_channel, c->mb_conn, c->mb_K, c->mb_c, c->mb_active, c->mb_wt, c->mb_bd + c0, c->mb_berr + c0);
            HIP_TRY(c, hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_mb_decide_batch, dim3((unsigned)n_agents), dim3(256), 0, c->stream, c->mb_bd, planes ? nullptr : c->mb_berr, A, d_fam, d_best,
                       d_flags);
    HIP_TRY(c, hipGetLastError());
    rc = packed_fetch(c, c->mb_res, C, n_agents);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    packed_unpack(c->mb_res, C, n_agents, angle_fam, best_heading, flags);
    return DV_OK;
}

extern "C" int dv_batch_mb_step_u8(dv_ctx* c, const uint8_t* planes, int n_agents, int n_headings, double* angle_fam, int32_t* best_heading) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_batch_mb_step_u8");
    if (rc) return rc;
    if (!planes || !angle_fam || !best_heading || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_batch_mb_step_u8: NULL argument, n_agents < 1 or n_headings < 1");
    return mb_batch(c, "dv_batch_mb_step_u8", planes, nullptr, nullptr, nullptr, n_agents, n_headings, nullptr, nullptr, angle_fam, best_heading, nullptr);
}

extern "C" int dv_batch_mb_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                      double* angle_fam, int32_t* best_heading, uint32_t* flags) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_batch_mb_sense_step");
    if (rc) return rc;
    if (!x || !y || !angles || !angle_fam || !best_heading || !flags || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_batch_mb_sense_step: NULL argument, n_agents < 1 or n_headings < 1");
    rc = sensor_fits(c, "dv_batch_mb_sense_step", c->mb_hh, c->mb_ww);
    if (rc) return rc;
    return mb_batch(c, "dv_batch_mb_sense_step", nullptr, x, y, angles, n_agents, n_headings, nullptr, nullptr, angle_fam, best_heading, flags);
}

extern "C" int dv_mb_read_weights(dv_ctx* c, uint8_t* out) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_mb_read_weights");
    if (rc) return rc;
    if (!out) return fail(c, DV_ERR_INVALID, "dv_mb_read_weights: out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->mb_wt, (size_t)c->mb_K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DV_OK;
}

extern "C" int dv_mb_set_weights(dv_ctx* c, const uint8_t* weights) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need_bank0(c, "dv_mb_set_weights");
    if (rc) return rc;
    if (!weights) return fail(c, DV_ERR_INVALID, "dv_mb_set_weights: weights is NULL");
    for (int k = 0; k < c->mb_K; ++k)
        if (weights[k] > 1) return fail(c, DV_ERR_INVALID, "dv_mb_set_weights: weights[%d] = %d is neither 0 nor 1", k, (int)weights[k]);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->mb_wt, weights, (size_t)c->mb_K, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // `weights` is borrowed for this call only
    return DV_OK;
}

extern "C" int dv_mb_info(dv_ctx* c, int* n_kc, int* n_pixels, int* fan_in, int* n_active, int64_t* views_trained, int64_t* n_depressed,
                          int64_t* bytes) {
    if (!c) return DV_ERR_INVALID;
    if (n_kc) *n_kc = c->mb_K;
    if (n_pixels) *n_pixels = c->mb_N;
    if (fan_in) *fan_in = c->mb_c;
    if (n_active) *n_active = c->mb_active;
    if (views_trained) *views_trained = c->mb_views[0];
    if (bytes) *bytes = (int64_t)c->mb_K;
    if (n_depressed) {
        *n_depressed = 0;
        if (c->mb_wt) {
            long long z = 0;
            HIP_TRY(c, hipSetDevice(c->device));
            if (c->mbp_pops) {                                // bank 0's, over the cells of its own population
                int rc = mbpop_count(c);
                if (rc) return rc;
            } else {
                hipLaunchKernelGGL(k_mb_count, dim3(1), dim3(256), 0, c->stream, c->mb_wt, c->mb_K, c->mb_zeros);
                HIP_TRY(c, hipGetLastError());
            }
            HIP_TRY(c, hipMemcpyAsync(&z, c->mb_zeros, sizeof z, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            *n_depressed = (int64_t)z;
        }
    }
    return DV_OK;
}

// ---- memory banks: n_banks memories behind the one connectivity (include/dejavu.h: dv_mbank_*) -------------------------------------
extern "C" int dv_mbank_set(dv_ctx* c, int n_banks) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_mbank_set");
    if (rc) return rc;
    if (n_banks < 1) return fail(c, DV_ERR_INVALID, "dv_mbank_set: n_banks %d < 1", n_banks);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_banks * (size_t)c->mb_K;
    unsigned char* wt = nullptr;
    long long* zeros = nullptr;
    hipError_t e = hipMalloc((void**)&wt, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&zeros, (size_t)n_banks * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(wt, 1, bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // (nothing enqueued reads the old weights any more)
    if (e != hipSuccess) {                                              // the model stays as it was
        (void)hipGetLastError();
        if (wt) (void)hipFree(wt);
        if (zeros) (void)hipFree(zeros);
        return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_mbank_set: %d banks of %d cells: %s", n_banks, c->mb_K, hipGetErrorString(e));
    }
    (void)hipFree(c->mb_wt);
    (void)hipFree(c->mb_zeros);
    c->mb_wt = wt;
    c->mb_zeros = zeros;
    c->mb_banks = n_banks;
    c->mb_views.assign((size_t)n_banks, 0);
    mbpop_drop(c);                                            // the banks are the begin's population's again
    return DV_OK;
}

extern "C" int dv_mbank_train_u8(dv_ctx* c, const uint8_t* planes, int64_t n, const int32_t* bank_of_view) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_mbank_train_u8");
    if (rc) return rc;
    if (!bank_of_view) return fail(c, DV_ERR_INVALID, "dv_mbank_train_u8: bank_of_view is NULL");
    return mb_train_u8(c, "dv_mbank_train_u8", planes, n, bank_of_view);
}

extern "C" int dv_mbank_train_from_poses(dv_ctx* c, const double* x, const double* y, const double* angle, int64_t n, const int32_t* bank_of_view,
                                         uint8_t* out_views) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_mbank_train_from_poses");
    if (rc) return rc;
    if (!bank_of_view) return fail(c, DV_ERR_INVALID, "dv_mbank_train_from_poses: bank_of_view is NULL");
    return mb_train_from_poses(c, "dv_mbank_train_from_poses", x, y, angle, n, bank_of_view, nullptr, out_views);
}

extern "C" int dv_lands_mbank_train_from_poses(dv_ctx* c, const double* x, const double* y, const double* angle, int64_t n, const int32_t* bank_of_view,
                                               const int32_t* land_of_view, uint8_t* out_views) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_lands_mbank_train_from_poses");
    if (rc) return rc;
    if (!bank_of_view || !land_of_view) return fail(c, DV_ERR_INVALID, "dv_lands_mbank_train_from_poses: bank_of_view or land_of_view is NULL");
    return mb_train_from_poses(c, "dv_lands_mbank_train_from_poses", x, y, angle, n, bank_of_view, land_of_view, out_views);
}

extern "C" int dv_mbank_step_u8(dv_ctx* c, const uint8_t* planes, int n_agents, int n_headings, const int32_t* bank_of_member, double* angle_fam,
                                int32_t* best_heading) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_mbank_step_u8");
    if (rc) return rc;
    if (!planes || !bank_of_member || !angle_fam || !best_heading || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_mbank_step_u8: NULL argument, n_agents < 1 or n_headings < 1");
    return mb_batch(c, "dv_mbank_step_u8", planes, nullptr, nullptr, nullptr, n_agents, n_headings, bank_of_member, nullptr, angle_fam, best_heading, nullptr);
}

extern "C" int dv_mbank_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                   const int32_t* bank_of_member, double* angle_fam, int32_t* best_heading, uint32_t* flags) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_mbank_sense_step");
    if (rc) return rc;
    if (!x || !y || !angles || !bank_of_member || !angle_fam || !best_heading || !flags || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_mbank_sense_step: NULL argument, n_agents < 1 or n_headings < 1");
    rc = sensor_fits(c, "dv_mbank_sense_step", c->mb_hh, c->mb_ww);
    if (rc) return rc;
    return mb_batch(c, "dv_mbank_sense_step", nullptr, x, y, angles, n_agents, n_headings, bank_of_member, nullptr, angle_fam, best_heading, flags);
}

extern "C" int dv_lands_mbank_sense_step(dv_ctx* c, const double* x, const double* y, const double* angles, int n_agents, int n_headings,
                                         const int32_t* bank_of_member, const int32_t* land_of_member, double* angle_fam, int32_t* best_heading,
                                         uint32_t* flags) {
    if (!c) return DV_ERR_INVALID;
    int rc = mb_need(c, "dv_lands_mbank_sense_step");
    if (rc) return rc;
    if (!x || !y || !angles || !bank_of_member || !land_of_member || !angle_fam || !best_heading || !flags || n_agents < 1 || n_headings < 1)
        return fail(c, DV_ERR_INVALID, "dv_lands_mbank_sense_step: NULL argument, n_agents < 1 or n_headings < 1");
    rc = sensor_fits(c, "dv_lands_mbank_sense_step", c->mb_hh, c->mb_ww);
    if (rc) return rc;
    return mb_batch(c, "dv_lands_mbank_sense_step", nullptr, x, y, angles, n_agents, n_headings, bank_of_member, land_of_member, angle_fam,
                    best_heading, flags);
}

static int mbank_one(dv_ctx* c, const char* who, int bank) {
    int rc = mb_need(c, who);
    if (rc) return rc;
    if (bank < 0 || bank >= c->mb_banks) return fail(c, DV_ERR_INVALID, "%s: bank %d outside [0, n_banks = %d)", who, bank, c->mb_banks);
    return DV_OK;
}

// Where bank `bank` lies in mb_wt and how long it is: n_kc of the model, or under a population table of the bank's own population.
static void mbank_span(const dv_ctx* c, int bank, size_t& off, size_t& len) {
    if (c->mbp_pops) { off = c->mbp_wt_off[(size_t)bank]; len = (size_t)c->mbp_K[(size_t)c->mbp_of_bank[(size_t)bank]]; }
    else { off = (size_t)bank * (size_t)c->mb_K; len = (size_t)c->mb_K; }
}

extern "C" int dv_mbank_read_weights(dv_ctx* c, int bank, uint8_t* out) {
    if (!c) return DV_ERR_INVALID;
    int rc = mbank_one(c, "dv_mbank_read_weights", bank);
    if (rc) return rc;
    if (!out) return fail(c, DV_ERR_INVALID, "dv_mbank_read_weights: out is NULL");
    size_t off, len;
    mbank_span(c, bank, off, len);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->mb_wt + off, len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DV_OK;
}

extern "C" int dv_mbank_set_weights(dv_ctx* c, int bank, const uint8_t* weights) {
    if (!c) return DV_ERR_INVALID;
    int rc = mbank_one(c, "dv_mbank_set_weights", bank);
    if (rc) return rc;
    if (!weights) return fail(c, DV_ERR_INVALID, "dv_mbank_set_weights: weights is NULL");
    size_t off, len;
    mbank_span(c, bank, off, len);
    for (size_t k = 0; k < len; ++k)
        if (weights[k] > 1) return fail(c, DV_ERR_INVALID, "dv_mbank_set_weights: weights[%d] = %d is neither 0 nor 1", (int)k, (int)weights[k]);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->mb_wt + off, weights, len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // `weights` is borrowed for this call only
    return DV_OK;
}

extern "C" int dv_mbank_info(dv_ctx* c, int* n_banks, int64_t* views_trained, int64_t* n_depressed) {
    if (!c) return DV_ERR_INVALID;
    const size_t B = (size_t)c->mb_banks;
    if (n_banks) *n_banks = c->mb_banks;
    if (views_trained) for (size_t b = 0; b < B; ++b) views_trained[b] = c->mb_views[b];
    if (n_depressed) {
        for (size_t b = 0; b < B; ++b) n_depressed[b] = 0;
        if (c->mb_wt) {
            std::vector<long long> z(B);
            HIP_TRY(c, hipSetDevice(c->device));
            if (c->mbp_pops) {                                // ragged banks: each over its own population's cells
                int rc = mbpop_count(c);
                if (rc) return rc;
            } else {
                hipLaunchKernelGGL(k_mb_count, dim3((unsigned)B), dim3(256), 0, c->stream, c->mb_wt, c->mb_K, c->mb_zeros);
                HIP_TRY(c, hipGetLastError());
            }
            HIP_TRY(c, hipMemcpyAsync(z.data(), c->mb_zeros, B * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (size_t b = 0; b < B; ++b) n_depressed[b] = (int64_t)z[b];
        }
    }
    return DV_OK;
}
