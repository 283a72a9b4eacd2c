// rt_trace3_body.inc -- the body of trace3_kernel (rt_trace.inc), included
// into its entry points: trace3_kernel<kMode, kFmt> (the two colour formats)
// and trace3_hit_kernel<kMode> (kFmt = RT_FORMAT_HIT).  The kernel's
// parameters, kMode and kFmt are in scope.  Not a standalone file.
    // (unsigned: the divisions by powers of two are shifts and masks)
    const unsigned bid = blockIdx.x;
    const int cbx = (int)(bid / kTiles), cby = (int)blockIdx.y;
    const int cb = cby * n_cx + cbx;
    const unsigned t = bid % kTiles;  // the tile of the bin (wave-uniform)
#if RT_TIMELINE
    const int tile = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
#endif
    const int lane = threadIdx.x & 63;
    const int n_tri = 12 * n_cubes;
    (void)n_tiles_x;
    (void)out_format;
    TL_MARK(tl0);
#if RT_TIMELINE
    const unsigned long long tlc0 = __builtin_amdgcn_s_memtime();
    unsigned tl1 = 0, tl2 = 0;
#endif
    const int rel_x = cbx * kCoarseW + (int)(t % kTilesX) * kWaveTile;
    const int rel_y = cby * kCoarseH + (int)(t / kTilesX) * kWaveTileH;  // vs row_begin
    const int tile_x = rel_x, tile_y = row_begin + rel_y;
    const int x = tile_x + (lane % kLanesX);  // the lane's pixel 0
    const int y0 = tile_y + (lane / kLanesX);
    // wave-uniform: tiles past the frame's right or bottom edge render nothing
    const bool tile_in = rel_x < width && rel_y < row_end - row_begin;

    // the bin's count (-1: non-finite scene data, see coarse3_kernel) is the
    // wave's first data load
#if RT_WALK_BALLOT == 2
    // issued beside the count's load, not after it: the list's first 64
    // entries (entry e on lane e; a bin's list holds half_cap entries)
    int spec_id = 0, spec_tm = 0;
    {
        const int* __restrict__ ids0 = lists + (int64_t)cb * kListStride * half_cap;
        const int* __restrict__ tms0 = ids0 + (1 + (int)(t / kTilesPerWord)) * half_cap;
        if (lane < half_cap) {
            spec_id = ids0[lane];
            spec_tm = tms0[lane];
        }
    }
#endif
    const int count_raw = kMode == 1 ? 0 : counts[cb];
    if (tile_in && kMode == 0 && count_raw < 0) {
        // Non-finite scene data: run the reference algorithm verbatim.
#pragma unroll 1
        for (int j = 0; j < kRowsPerLane; ++j) {
            const int xj = x + pix_dx(j), y = y0 + pix_dy(j);
            if (xj < width && y < row_end)
                store_fmt<kFmt>(out, (int64_t)(y - row_begin) * width + xj,
                                collide_generic<kFmt>(scene, make_float4((float)xj, (float)y, 0.0f, 1.0f),
                                                dir));
        }
    } else if (tile_in) {
    int4v pix[kRowsPerLane];  // assigned after the walk (not live during it)
    float closest[kRowsPerLane];
    int hit[kRowsPerLane];
    double px[kRowsPerLane], py[kRowsPerLane];
    float pxf[kRowsPerLane], pyf[kRowsPerLane];
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        closest[j] = kFar;
        hit[j] = -1;
        py[j] = (double)(y0 + pix_dy(j));
        pyf[j] = (float)(y0 + pix_dy(j));
        px[j] = (double)(x + pix_dx(j));
        pxf[j] = (float)(x + pix_dx(j));
    }
#if RT_DEPTH_CULL
    // order_key of the largest `closest` in the tile, refreshed lazily
    unsigned tile_max_key = order_key(kFar);
    bool dirty = false;
#endif
    const int count = count_raw < 0 ? 0 : count_raw;
    const int* __restrict__ ids = lists + (int64_t)cb * kListStride * half_cap;
    const int* __restrict__ tms = ids + (1 + (int)(t / kTilesPerWord)) * half_cap;  // its word
    const int tm_shift = kTileBits * (int)(t % kTilesPerWord);
#if RT_TIMELINE
    tl1 = rt_now();
#endif
#if RT_WALK_BALLOT
    // The bin's list 64 entries at a time as vector loads (entry e on lane
    // e), this tile's keep bits in one ballot, and only the kept entries
    // visited (s_ff1 over the mask, id and bits by v_readlane): the walk no
    // longer spends scalar instructions on the bin's entries this tile does
    // not keep (most of them), in primitive order as before.
    for (int c0 = 0; c0 < count; c0 += 64) {
        const int e = c0 + lane;
        int idl = 0;
        unsigned bl = 0u;
        if (e < count) {
#if RT_WALK_BALLOT == 2
            idl = c0 == 0 ? spec_id : ids[e];
            bl = ((unsigned)(c0 == 0 ? spec_tm : tms[e]) >> tm_shift) & kTileMask;
#else
            idl = ids[e];
            bl = ((unsigned)tms[e] >> tm_shift) & kTileMask;
#endif
        }
        unsigned long long keep = __ballot((bl & kKeepMask) != 0u);
        while (keep) {
            const int k = __builtin_ctzll(keep);
            keep &= keep - 1ull;
            const int p = __builtin_amdgcn_readlane(idl, k);
            const unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)bl, k);
            if (kMode == 2) {
                hit[0] = hit[0] > p ? hit[0] : -1;
                continue;
            }
            // both branches produce t per row (NaN: may not take); closest
            // and hit are updated once, after them (round 4: trace 1-3 %
            // faster than a test-and-update in each branch, DESIGN.md §3.5)
            float tc[kRowsPerLane];
            int slot;
            if (p < n_tri) {
                const TriRec r = tri_at(tri, p);
                asm volatile("" ::"s"(r.p0), "s"(r.p1), "s"(r.dz));
                if constexpr (kRecomputeXY)
                    tri_rows_fresh(r, bits, px[0], py[0], tc);
                else
                    tri_rows(r, bits, px, py, tc);
                slot = p / 12;
            } else {
                const SphRec r = sph_at(sph, p - n_tri);
#if RT_DEPTH_CULL
                // t0 >= tmin >= every closest: no lane can take it (strict <)
                if (dirty) {
                    tile_max_key = wave_max_key(closest);
                    dirty = false;
                }
                if (r.tmin_key >= tile_max_key) continue;
#endif
                if constexpr (kRecomputeXY)
                    sph_rows_fresh(r, bits, pxf[0], pyf[0], tc);
                else
                    sph_rows(r, bits, pxf, pyf, tc);
                slot = n_cubes + (p - n_tri);
            }
            take_rows(tc, slot, closest, hit);
#if RT_DEPTH_CULL
            dirty = true;
#endif
        }
    }
#else
    for (int i0 = 0; i0 < count; i0 += 8) {
        int idv[8], tmv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            idv[k] = ids[i0 + k];  // half_cap is a multiple of 8 past the count
            tmv[k] = tms[i0 + k];
        }
        const int n = min(8, count - i0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= n) break;
            const unsigned bits = ((unsigned)tmv[k] >> tm_shift) & kTileMask;
            if (!(bits & kKeepMask)) continue;
            const int p = idv[k];
            if (kMode == 2) {
                hit[0] = hit[0] > p ? hit[0] : -1;
                continue;
            }
            // both branches produce t per row (NaN: may not take); closest
            // and hit are updated once, after them (round 4: trace 1-3 %
            // faster than a test-and-update in each branch, DESIGN.md §3.5)
            float tc[kRowsPerLane];
            int slot;
            if (p < n_tri) {
                const TriRec r = tri_at(tri, p);
                asm volatile("" ::"s"(r.p0), "s"(r.p1), "s"(r.dz));
                if constexpr (kRecomputeXY)
                    tri_rows_fresh(r, bits, px[0], py[0], tc);
                else
                    tri_rows(r, bits, px, py, tc);
                slot = p / 12;
            } else {
                const SphRec r = sph_at(sph, p - n_tri);
#if RT_DEPTH_CULL
                // t0 >= tmin >= every closest: no lane can take it (strict <)
                if (dirty) {
                    tile_max_key = wave_max_key(closest);
                    dirty = false;
                }
                if (r.tmin_key >= tile_max_key) continue;
#endif
                if constexpr (kRecomputeXY)
                    sph_rows_fresh(r, bits, pxf[0], pyf[0], tc);
                else
                    sph_rows(r, bits, pxf, pyf, tc);
                slot = n_cubes + (p - n_tri);
            }
            take_rows(tc, slot, closest, hit);
#if RT_DEPTH_CULL
            dirty = true;
#endif
        }
    }
#endif
#if RT_TIMELINE
    tl2 = rt_now();
#endif
#if RT_EXTRA_VALU || RT_EXTRA_SALU
    {
        // diagnostics only (scripts/variants.sh): RT_EXTRA_VALU extra VALU /
        // RT_EXTRA_SALU extra SALU instructions per wave, to price issue in
        // this kernel (DESIGN.md §3.3)
        float xa = closest[0], xb = closest[1];
#pragma unroll
        for (int q = 0; q < RT_EXTRA_VALU / 2; ++q) {
            asm volatile("v_add_f32 %0, %0, %1" : "+v"(xa) : "v"(xb));
            asm volatile("v_add_f32 %0, %0, %1" : "+v"(xb) : "v"(xa));
        }
        unsigned sa = (unsigned)count, sb = (unsigned)cb;
#pragma unroll
        for (int q = 0; q < RT_EXTRA_SALU / 2; ++q) {
            asm volatile("s_add_u32 %0, %0, %1" : "+s"(sa) : "s"(sb));
            asm volatile("s_add_u32 %0, %0, %1" : "+s"(sb) : "s"(sa));
        }
        if (xa == 1234.5f && xb == 1234.5f && sa == 7u) hit[0] = -2;  // never (keeps the chains)
    }
#endif
    shade_pixels<kMode, kFmt>(colours, closest, hit, pix);
    const bool full = rel_x + kWaveTile <= width && tile_y + kWaveTileH <= row_end;
    store_rows<kMode, kFmt>(pix, rel_x, rel_y, lane, width, row_end - row_begin, full, out);
    }  // finite scene, tile inside the frame
#if RT_TIMELINE
    {
        const unsigned tl3 = rt_now();
        const unsigned long long tlc3 = __builtin_amdgcn_s_memtime();
        if (lane == 0) {
            unsigned* o = g_timeline + 8 * (int64_t)tile;
            o[0] = tl0; o[1] = tl1; o[2] = tl2; o[3] = tl3;
            o[4] = (unsigned)tlc0; o[5] = (unsigned)tlc3;
            o[6] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            o[7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        }
    }
#endif
