// orb_pyramid_kernels.inc -- the two pyramid builders, included twice by
// orb_kernels.hpp: PLVI_PYR_AREA 0 defines orb_pyramid_kernel /
// orb_resize_level_kernel where they always stood, PLVI_PYR_AREA 1 the
// *_area kernels of exact-half levels (kPyrXtabAreaTail) after the last
// kernel of the file.  Plain textual inclusion, so both variants come from
// one text; the pixel arithmetic itself (pyr_quad, pyr_row_quads,
// pyr_store_quad) is shared by the two builders and lives in orb_kernels.hpp.
__global__ __launch_bounds__(64 * (kPyrFrames + 1)) __attribute__((amdgpu_waves_per_eu(PLVI_PYR_WPE))) void PLVI_PYR_KERNEL(
    const OrbLevelDev* __restrict__ lvs, int L, const uint8_t* __restrict__ frames, size_t f_frame, size_t f_row,
    int nf, uint8_t* __restrict__ pyr, const uint32_t* __restrict__ xtab, int xtab_n, int frame_lds, int generic) {
    PLVI_ORB_PRIO_SET();
    extern __shared__ __align__(16) uint8_t lds_pyr_g[];
    __shared__ int s_w[kOrbMaxLevels], s_h[kOrbMaxLevels], s_roff[kOrbMaxLevels], s_xoff[kOrbMaxLevels];
    __shared__ int s_wide[kOrbMaxLevels];  // the level's quads do not fit the 8-byte tap window (kPyrXtabWide)
    __shared__ double s_sy[kOrbMaxLevels];
    __shared__ int s_cnt[2 * kPyrFrames];  // per frame: rows loaded, rows consumed
    __shared__ uint8_t* s_dbase[kPyrFrames][kOrbMaxLevels];  // per resizer wave: its frame's level planes
    __shared__ int s_prod[kPyrFrames][kOrbMaxLevels];        // and the rows it has produced per level
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform: scalar role / frame
    const int f0 = blockIdx.x * kPyrFrames;
    const int nfw = min(kPyrFrames, nf - f0);  // frames of this workgroup
    lds_u32* ltab = (lds_u32*)lds_pyr_g;     // column table first (xtab_n words)
    if (threadIdx.x < L) {
        s_w[threadIdx.x] = lvs[threadIdx.x].w;
        s_h[threadIdx.x] = lvs[threadIdx.x].h;
        s_sy[threadIdx.x] = lvs[threadIdx.x].rsy;
        s_xoff[threadIdx.x] = lvs[threadIdx.x].xtab;
        s_wide[threadIdx.x] = threadIdx.x > 0 && (xtab[lvs[threadIdx.x].xtab] & kPyrXtabWide);
    }
    if (threadIdx.x == 0) {
        int o = kPyrRing * ((lvs[0].w + 3) & ~3);  // level-0 ring first
        s_roff[0] = 0;
        for (int l = 1; l < L - 1; ++l) {
            s_roff[l] = o;
            o += 2 * ((lvs[l].w + 3) & ~3);
        }
    }
    if (threadIdx.x < 2 * kPyrFrames) s_cnt[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < xtab_n; i += 64 * (kPyrFrames + 1)) ltab[i] = xtab[i];
    __syncthreads();  // the only workgroup barrier
    const int W0 = s_w[0], H0 = s_h[0];
    const int pitch0 = (W0 + 3) & ~3;
    lds_u8* fbase = (lds_u8*)(lds_pyr_g + 4 * xtab_n);  // per-frame regions of frame_lds bytes
    if (wave == 0) {
        // ------------------------------------------------ loader
        const int nd = (W0 + 3) >> 2;
        bool al4 = (W0 & 3) == 0 && (f_row & 3) == 0 && (f_frame & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(frames) & 3) == 0;
        auto load_row = [&](int k, int r, uint32_t* v) {
            const uint8_t* row = frames + (size_t)(f0 + k) * f_frame + (size_t)r * f_row;
            if (al4) {
                const uint32_t* rw = reinterpret_cast<const uint32_t*>(row);
#pragma unroll
                for (int q = 0; q < kPyrDw; ++q)
                    v[q] = lane + 64 * q < nd ? __builtin_nontemporal_load(rw + lane + 64 * q) : 0u;
            } else {
#pragma unroll
                for (int q = 0; q < kPyrDw; ++q) {
                    const int d = lane + 64 * q;
                    uint32_t x = 0;
                    for (int b = 0; b < 4; ++b)
                        if (4 * d + b < W0) x |= (uint32_t)row[4 * d + b] << (8 * b);
                    v[q] = x;
                }
            }
        };
        uint32_t pf[kPyrAhead][kPyrFrames][kPyrDw];
#pragma unroll
        for (int j = 0; j < kPyrAhead; ++j)
#pragma unroll
            for (int k = 0; k < kPyrFrames; ++k)
                if (j < H0 && k < nfw) load_row(k, j, pf[j][k]);
        for (int rb = 0; rb < H0; rb += kPyrAhead) {
#pragma unroll
            for (int j = 0; j < kPyrAhead; ++j) {
                const int r = rb + j;
                if (r >= H0) break;
#pragma unroll
                for (int k = 0; k < kPyrFrames; ++k) {
                    if (k >= nfw) break;
                    lds_i32* loaded = (lds_i32*)&s_cnt[2 * k];
                    lds_i32* consumed = (lds_i32*)&s_cnt[2 * k + 1];
                    // the resizer needs rows consumed-1 and consumed: slot r % ring is free once r - ring <= consumed - 2
                    while (r - kPyrRing > lds_load_acquire(consumed) - 2) __builtin_amdgcn_s_sleep(1);
                    lds_u32* slot = (lds_u32*)(fbase + (size_t)k * frame_lds + (r % kPyrRing) * pitch0);
#pragma unroll
                    for (int q = 0; q < kPyrDw; ++q)
                        if (lane + 64 * q < nd) slot[lane + 64 * q] = pf[j][k][q];
                    lds_publish(loaded, r + 1, lane);
                    if (r + kPyrAhead < H0) load_row(k, r + kPyrAhead, pf[j][k]);
                }
            }
        }
        return;
    }
    // ---------------------------------------------------- resizer of frame f
    const int k = wave - 1;
    if (k >= nfw) return;
    const int f = f0 + k;
    lds_u8* lds_pyr = fbase + (size_t)k * frame_lds;
    lds_i32* s_loaded = (lds_i32*)&s_cnt[2 * k];
    lds_i32* s_consumed = (lds_i32*)&s_cnt[2 * k + 1];
    // this frame's level planes and rows produced per level: in LDS, written and
    // read by this wave alone (registers indexed by the level cost a 16-way
    // select per visit; no global parameter loads inside the row loop)
    if (lane < kOrbMaxLevels) {
        s_dbase[k][lane] = lane < L ? pyr + lvs[lane].off + (size_t)f * lvs[lane].plane : nullptr;
        s_prod[k][lane] = 0;
    }
    wave_sync();
    for (int r = 0; r < H0; ++r) {
        while (lds_load_acquire(s_loaded) <= r) __builtin_amdgcn_s_sleep(1);
        int avail = r + 1;  // rows of the source level available
        for (int l = 1; l < L; ++l) {
            const int sh = s_h[l - 1], w = s_w[l], h = s_h[l];
            const int spitch = (s_w[l - 1] + 3) & ~3, pitch = (w + 3) & ~3;
            const int sring = l == 1 ? kPyrRing : 2;
            const double scy = s_sy[l];
            const lds_u32* T = ltab + s_xoff[l];
            int y = __builtin_amdgcn_readfirstlane(s_prod[k][l]);
            const int y_start = y;
            while (y < h) {
                float fy = (float)((y + 0.5) * scy - 0.5);
                int sy = (int)fy;
                sy -= (sy > fy);
                fy -= (float)sy;
                const int r1 = min(max(sy + 1, 0), sh - 1);
                if (r1 >= avail) break;
                const int r0 = min(max(sy, 0), sh - 1);
                const unsigned b0 = (unsigned)__builtin_rintf((1.f - fy) * 2048),
                               b1 = (unsigned)__builtin_rintf(fy * 2048);
                const lds_u8* S0 = lds_pyr + s_roff[l - 1] + (r0 % sring) * spitch;
                const lds_u8* S1 = lds_pyr + s_roff[l - 1] + (r1 % sring) * spitch;
                uint8_t* D = s_dbase[k][l] + (size_t)y * w;
                lds_u8* R = l < L - 1 ? lds_pyr + s_roff[l] + (y & 1) * pitch : nullptr;
                // four consecutive pixels per lane (pyr_row_quads, orb_kernels.hpp); the
                // row's last quad never stores past column w - 1 in HBM (pyr_store_quad)
                if (s_wide[l])
                    pyr_row_pixels<PLVI_PYR_AREA>(T, S0, S1, D, R, w, lane, b0, b1, generic);
                else if (generic)
                    pyr_row_quads<PLVI_PYR_AREA, true>(T, S0, S1, (spitch >> 2) - 1, D, R, w, lane, b0, b1);
                else
                    pyr_row_quads<PLVI_PYR_AREA, false>(T, S0, S1, (spitch >> 2) - 1, D, R, w, lane, b0, b1);
                ++y;
                // one wave: its LDS row writes precede the next level's reads in
                // program order (compiler ordering point only)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            if (lane == 0) s_prod[k][l] = y;
            if (y == y_start) break;  // nothing new at level l: deeper levels have no new source rows
            avail = y;
        }
        lds_publish(s_consumed, r + 1, lane);
    }
}

// ---------------------------------------------------------------------------
// K1a', small batches: one launch per level (level l from level l-1 in HBM /
// L2), thread = 4 consecutive output pixels of one row, the whole chip on
// every level.  The streaming kernel above runs one resizer wave per frame
// through all 7 chained levels: at one frame that is a 2.3 ms serial chain
// for 1.6 MB (DESIGN.md §4).  Same quad routine (pyr_quad), same packed
// column table, same 8U / generic switch.  Level 1 reads the caller's frames (level 0's
// plane is written later by orb_blur_fast_kernel).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void PLVI_RESIZE_KERNEL(const uint8_t* __restrict__ src, size_t s_frame,
                                                               size_t s_row, int sw, int sh, uint8_t* __restrict__ dst,
                                                               size_t d_frame, int w, int h, double scy,
                                                               const uint32_t* __restrict__ T, int generic,
                                                               uint32_t qinv) {
    PLVI_ORB_PRIO_SET();
    const int qpr = (w + 3) >> 2;  // quads per row
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= qpr * h) return;
    const int f = blockIdx.y;
    // i / qpr by the host's qinv = ceil(2^32 / qpr): exact while i * (qinv * qpr - 2^32) < 2^32 (pyr_qinv)
    const int y = (int)__umulhi((uint32_t)i, qinv), x0 = (i - y * qpr) * 4;
    float fy = (float)((y + 0.5) * scy - 0.5);
    int sy = (int)fy;
    sy -= (sy > fy);
    fy -= (float)sy;
    const int r0 = min(max(sy, 0), sh - 1), r1 = min(max(sy + 1, 0), sh - 1);
    const unsigned b0 = (unsigned)__builtin_rintf((1.f - fy) * 2048), b1 = (unsigned)__builtin_rintf(fy * 2048);
    const uint8_t* S0 = src + (size_t)f * s_frame + (size_t)r0 * s_row;
    const uint8_t* S1 = src + (size_t)f * s_frame + (size_t)r1 * s_row;
    uint8_t* D = dst + (size_t)f * d_frame + (size_t)y * w;
    // the level's entries are padded to whole quads and start 16-byte aligned
    const pyr_u32x4 q = *reinterpret_cast<const pyr_u32x4*>(T + x0);
    const uint32_t e[4] = {q.x, q.y, q.z, q.w};
    uint32_t pk;
    if (e[0] & kPyrXtabWide) {
        pk = generic ? pyr_quad_pixels<PLVI_PYR_AREA, true>(e, S0, S1, b0, b1)
                     : pyr_quad_pixels<PLVI_PYR_AREA, false>(e, S0, S1, b0, b1);
    } else {
        // the quad's taps lie in the 8 bytes from its first sx on; the window is
        // held inside the source row (sw >= 8: append_xtab), which keeps every tap
        const int sxb = min((int)(e[0] & 1023u), sw - 8);
        const uint32_t lo0 = ld_u32(S0 + sxb), hi0 = ld_u32(S0 + sxb + 4), lo1 = ld_u32(S1 + sxb),
                       hi1 = ld_u32(S1 + sxb + 4);
        pk = generic ? pyr_quad<PLVI_PYR_AREA, true>(e, (unsigned)sxb, lo0, hi0, lo1, hi1, b0, b1)
                     : pyr_quad<PLVI_PYR_AREA, false>(e, (unsigned)sxb, lo0, hi0, lo1, hi1, b0, b1);
    }
    pyr_store_quad(D, x0, w, pk);  // the row's last quad never stores past column w - 1
}
