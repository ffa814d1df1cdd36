// The landscape generator's heat equation on the device (include/dejavu.h: dv_diffuse_*).  The reference's diffuse
// (navsim/util.pyx:189-235) is the explicit five-point scheme under periodic boundaries, in double, one full sweep per step:
//
//     new[i,j] = m[i,j] + multiplier * ((((m[i+1,j] + m[i-1,j]) - 4*m[i,j]) + m[i,j+1]) + m[i,j-1])
//
// Both kernels below evaluate exactly this expression, every operation rounded on its own (the file is built with
// -ffp-contract=off and the bodies say so again: an fma in `m + multiplier * s` would change the last bit), so their results carry
// the reference's bits whatever the launch geometry.
//
//   k_diffuse_plain    one step per launch from one buffer into the other: 8 B read (neighbours come from cache) + 8 B written per
//                      cell and step.  The A/B baseline.
//   k_diffuse_blocked  temporal blocking: a workgroup loads an S x S window of the field -- its B x B tile, B = S - 2T, plus a halo
//                      of depth T, indices wrapped with a true modulo (T may exceed the side: a window then holds several copies of
//                      the field, which is what the periodic boundary means) -- into LDS, advances it `steps` <= T steps between two
//                      LDS copies and stores the tile.  After step s only the cells at least s away from the window's edge are
//                      right (their neighbours were right after step s-1), so the computed square shrinks ring by ring and the tile
//                      in the middle is exact after up to T steps.  Every cell, halo or not, is the same expression on the same
//                      values as in the plain form, so the forms agree bit for bit.  Traffic per T steps: S*S doubles read and B*B
//                      written per tile.
namespace dv {

__device__ __forceinline__ int wrap_index(int g, int n) {
    g %= n;
    return g < 0 ? g + n : g;
}

__global__ __launch_bounds__(256) void k_diffuse_plain(const double* __restrict__ src, double* __restrict__ dst, int n, double mult) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n) return;
    const int ip = i + 1 == n ? 0 : i + 1, im = i == 0 ? n - 1 : i - 1;
    const int jp = j + 1 == n ? 0 : j + 1, jm = j == 0 ? n - 1 : j - 1;
    const size_t row = (size_t)i * (size_t)n;
    const double mid = src[row + j];
    double s = src[(size_t)ip * n + j] + src[(size_t)im * n + j];
    s = s - 4.0 * mid;
    s = s + src[row + jp];
    s = s + src[row + jm];
    dst[row + j] = mid + mult * s;
}

// S: side of the LDS window; R: rows per thread (a thread owns one column of a strip of R rows and carries the column's three
// values in registers while it walks down).  Threads: S * (S / R), thread t on column t % S of strip t / S.  LDS: 2 * S * S doubles.
template <int S, int R>
__global__ __launch_bounds__(S * (S / R)) void k_diffuse_blocked(const double* __restrict__ src, double* __restrict__ dst, int n, int T,
                                                                  int steps, double mult) {
#pragma clang fp contract(off)
    static_assert(S % R == 0 && S * (S / R) <= 1024, "window shape");
    extern __shared__ double dwin[];                 // [2][S][S]
    const int B = S - 2 * T;
    const int x = (int)threadIdx.x % S, ys = ((int)threadIdx.x / S) * R;
    const int gx0 = (int)blockIdx.x * B - T, gy0 = (int)blockIdx.y * B - T;
    {
        const int gx = wrap_index(gx0 + x, n);
        for (int r = 0; r < R; ++r) {
            const int gy = wrap_index(gy0 + ys + r, n);
            dwin[(ys + r) * S + x] = src[(size_t)gy * (size_t)n + gx];
        }
    }
    __syncthreads();
    double* cur = dwin;
    double* nxt = dwin + S * S;
    for (int s = 1; s <= steps; ++s) {
        const int lo = s, hi = S - s;                // this step leaves [lo, hi) x [lo, hi) right
        const int y0 = ys > lo ? ys : lo, y1 = ys + R < hi ? ys + R : hi;
        if (x >= lo && x < hi && y0 < y1) {
            double up = cur[(y0 - 1) * S + x], mid = cur[y0 * S + x];
            for (int y = y0; y < y1; ++y) {
                const double dn = cur[(y + 1) * S + x];
                double v = dn + up;
                v = v - 4.0 * mid;
                v = v + cur[y * S + x + 1];
                v = v + cur[y * S + x - 1];
                nxt[y * S + x] = mid + mult * v;
                up = mid;
                mid = dn;
            }
        }
        __syncthreads();
        double* t = cur; cur = nxt; nxt = t;
    }
    if (x >= T && x < T + B && gx0 + x < n) {
        for (int r = 0; r < R; ++r) {
            const int y = ys + r;
            if (y >= T && y < T + B && gy0 + y < n) dst[(size_t)(gy0 + y) * (size_t)n + (size_t)(gx0 + x)] = cur[y * S + x];
        }
    }
}

}  // namespace dv

static constexpr int kDiffuseT = 8;              // steps per launch of the blocked form (with the 64 window: by measurement)
static constexpr int kDiffuseMaxSide = 32768;    // 8 GiB per buffer

static void diffuse_free(dv_ctx* c) {
    for (double*& p : c->d_diff) if (p) { (void)hipFree(p); p = nullptr; }
    c->diff_n = 0;
    c->diff_cur = 0;
    c->diff_done = 0;
}

// window side and steps per launch of the blocked form: dv_diffuse_configure, else DEJAVU_DIFFUSE_S / DEJAVU_DIFFUSE_T, else the default
static void diffuse_shape(const dv_ctx* c, int* S, int* T) {
    *S = c->diff_S == 96 ? 96 : 64;
    *T = c->diff_T > 0 ? c->diff_T : kDiffuseT;
    if (2 * *T > *S - 8) *T = (*S - 8) / 2;
}

template <int S, int R>
static int launch_diffuse_blocked(dv_ctx* c, const double* src, double* dst, int T, int steps) {
    const size_t lds = 2 * (size_t)S * S * sizeof(double);
    if (lds > 64 * 1024 && !c->diff_lds_opted) {                 // once per context: more than 64 KB of LDS has to be asked for
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_diffuse_blocked<S, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->diff_lds_opted = true;
    }
    const int B = S - 2 * T, tiles = (c->diff_n + B - 1) / B;
    hipLaunchKernelGGL((k_diffuse_blocked<S, R>), dim3((unsigned)tiles, (unsigned)tiles), dim3(S * (S / R)), lds, c->stream, src, dst, c->diff_n, T,
                       steps, c->diff_mult);
    HIP_TRY(c, hipGetLastError());
    return DV_OK;
}

extern "C" int dv_diffuse_configure(dv_ctx* c, int window, int steps_per_launch) {
    if (!c) return DV_ERR_INVALID;
    if ((window != 0 && window != 64 && window != 96) || steps_per_launch < 0 || steps_per_launch > 44)
        return fail(c, DV_ERR_INVALID, "dv_diffuse_configure: window %d (0, 64 or 96), steps per launch %d (0..44)", window, steps_per_launch);
    if (window) c->diff_S = window;
    if (steps_per_launch) c->diff_T = steps_per_launch;
    return DV_OK;
}

extern "C" int dv_diffuse_begin(dv_ctx* c, const double* init, int n, double cc, double delta_t_factor) {
    if (!c) return DV_ERR_INVALID;
    if (!init) return fail(c, DV_ERR_INVALID, "dv_diffuse_begin: the field is NULL");
    if (n < 1 || n > kDiffuseMaxSide) return fail(c, DV_ERR_INVALID, "dv_diffuse_begin: side %d outside 1..%d", n, kDiffuseMaxSide);
    if (cc == 0.0) return fail(c, DV_ERR_INVALID, "dv_diffuse_begin: c is 0 (the reference divides by it)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    diffuse_free(c);
    const size_t bytes = (size_t)n * (size_t)n * sizeof(double);
    for (double*& p : c->d_diff) {
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) {
            diffuse_free(c);
            return fail(c, e == hipErrorOutOfMemory ? DV_ERR_OOM : DV_ERR_HIP, "dv_diffuse_begin: %s", hipGetErrorString(e));
        }
    }
    // navsim/util.pyx:206-209, in its order of operations
    const double delta_s = 1.0 / (double)(n + 1);
    const double delta_t = delta_t_factor * ((delta_s * delta_s) / (2 * cc));
    c->diff_mult = cc * (delta_t / (delta_s * delta_s));
    hipError_t e = hipMemcpyAsync(c->d_diff[0], init, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // `init` is borrowed for this call only
    if (e != hipSuccess) {
        diffuse_free(c);                                       // no field rather than one of uninitialised memory
        return fail(c, DV_ERR_HIP, "dv_diffuse_begin: upload: %s", hipGetErrorString(e));
    }
    c->diff_n = n;
    return DV_OK;
}

extern "C" int dv_diffuse_advance(dv_ctx* c, int64_t nstep, uint32_t flags) {
    if (!c) return DV_ERR_INVALID;
    if (nstep < 0 || flags > DV_DIFFUSE_BLOCKED) return fail(c, DV_ERR_INVALID, "dv_diffuse_advance: bad step count or flags");
    if (c->diff_n < 1) return fail(c, DV_ERR_STATE, "dv_diffuse_advance: no field (dv_diffuse_begin first)");
    HIP_TRY(c, hipSetDevice(c->device));
    int S, T;
    diffuse_shape(c, &S, &T);
    const int n = c->diff_n;
    // DV_DIFFUSE_AUTO is the blocked form: it measured faster than the plain one at 2000 x 2000 x 2000 steps and at 500 x 500
    // (DESIGN 4).  DEJAVU_DIFFUSE_AUTO=1 makes it the plain form (A/B).
    const bool blocked = flags == DV_DIFFUSE_BLOCKED || (flags == DV_DIFFUSE_AUTO && c->diff_auto_env != 1);
    int64_t left = nstep;
    while (left > 0) {
        const double* src = c->d_diff[c->diff_cur];
        double* dst = c->d_diff[c->diff_cur ^ 1];
        int k = 1;
        if (blocked) {
            k = left < T ? (int)left : T;
            const int rc = S == 64 ? launch_diffuse_blocked<64, 8>(c, src, dst, T, k) : launch_diffuse_blocked<96, 12>(c, src, dst, T, k);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(k_diffuse_plain, dim3((unsigned)((n + 63) / 64), (unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, src, dst, n,
                               c->diff_mult);
            HIP_TRY(c, hipGetLastError());
        }
        c->diff_cur ^= 1;
        c->diff_done += k;
        left -= k;
    }
    return DV_OK;
}

extern "C" int dv_diffuse_read(dv_ctx* c, double* out) {
    if (!c) return DV_ERR_INVALID;
    if (!out) return fail(c, DV_ERR_INVALID, "dv_diffuse_read: out is NULL");
    if (c->diff_n < 1) return fail(c, DV_ERR_STATE, "dv_diffuse_read: no field (dv_diffuse_begin first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->d_diff[c->diff_cur], (size_t)c->diff_n * (size_t)c->diff_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DV_OK;
}

extern "C" int dv_diffuse_end(dv_ctx* c) {
    if (!c) return DV_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    diffuse_free(c);
    return DV_OK;
}

extern "C" int dv_diffuse_info(dv_ctx* c, int* tile, int* steps_per_launch, int* steps_done) {
    if (!c) return DV_ERR_INVALID;
    int S, T;
    diffuse_shape(c, &S, &T);
    if (tile) *tile = S - 2 * T;
    if (steps_per_launch) *steps_per_launch = T;
    if (steps_done) *steps_done = (int)(c->diff_done > 0x7fffffff ? 0x7fffffff : c->diff_done);
    return DV_OK;
}

extern "C" int dv_diffuse(dv_ctx* c, const double* init, int n, int64_t nstep, double cc, double delta_t_factor, uint32_t flags, double* out) {
    if (!c) return DV_ERR_INVALID;
    if (!out) return fail(c, DV_ERR_INVALID, "dv_diffuse: out is NULL");
    int rc = dv_diffuse_begin(c, init, n, cc, delta_t_factor);
    if (!rc) rc = dv_diffuse_advance(c, nstep, flags);
    if (!rc) rc = dv_diffuse_read(c, out);
    const std::string err = c->err;
    const int rc_end = dv_diffuse_end(c);
    if (rc) { c->err = err; return rc; }
    return rc_end;
}
