// pjd_k_lanes_parse_body.h -- set-up and entry parser of one back-end range of the lane streams, included textually by
// pjd_idct_range (pjd_k_backend.hip), the plane kernel of the libjpeg-exact mode (pjd_k_backend_std.hip) and the grey lane kernels; textual inclusion
// for the reason pjd_k_idct_dense_body.h gives.  Uses B, iwg, tile, qz, mcu_xy, comp_of, du_head, wagg, ltab of the including
// function and leaves wg, im, tid, lane, wv, dus, nl, n_du, n_valid and pred0 behind.  With PJD_LANES_RAW defined the tile receives the
// coefficients as decoded (quantiser 1, DC differences likewise) instead of their 16-bit products.  With PJD_LANES_LUMA_ONLY defined
// (the grey back end, pjd_k_backend_gray.hip) the entries of chroma units are walked -- the stream interleaves them -- and dropped.
#ifdef PJD_LANES_LUMA_ONLY
#define PJD_LANES_KEEP(u) (comp_of[u] == 0)
#else
#define PJD_LANES_KEEP(u) true
#endif
    const PjdDevIdctWg wg = B.iwgs[iwg];
    const PjdDevImage &im = B.images[wg.image];
    if ((im.flags & PJD_IF_SEQUENTIAL) || (B.status[wg.image] & PJD_STW_NEEDS_EXACT)) return;   // the dense path redoes it
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t dus = im.dus_per_mcu, nl = im.n_luma;
    const uint32_t n_du = wg.n_mcu * dus;
    const uint32_t RI = im.restart_interval;

    const bool quirk = !(im.flags & PJD_IF_STANDARD_ZIGZAG);    // the reference's zigzag_map[48] = 38 (default)
    // The reference's zigzag quirk: slots 48 AND 52 land on natural position 38, and the later one -- slot 52, even an explicit zero --
    // wins.  Entries of one unit may be parsed by two threads, so slot 52 is parked in the first padding cell of the unit's tile row
    // (position 64, raw value: quantiser 1; the cell starts as PJD_COEF_SENTINEL = "no slot 52 in this unit") and moved over
    // position 38 when the rows are done.
    if (tid < 192) {
        const uint32_t nat = (!quirk && (tid & 63) == 48) ? 58u : c_zz[tid & 63];
#ifdef PJD_LANES_RAW
        uint32_t v = 1u | (nat << 16);
#else
        uint32_t v = (uint32_t)B.qtab[(size_t)wg.image * 192 + (tid & ~63u) + nat] | (nat << 16);
#endif
        if (quirk && (tid & 63) == 52) v = 1u | (64u << 16);
        qz[tid >> 6][tid & 63] = v;
    }
    // unvisited positions are zero (the reference's buffers start zeroed); a row is 9 x 16 bytes, the last of them padding
    static_assert(TILE_STRIDE == 72, "the padding cell of a tile row is element 64");
    // (row, 16-byte column) by shift and mask: eight zero stores per row, then the row's padding
    for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS)
        *reinterpret_cast<uint4 *>(&tile[i >> 3][(i & 7) * 8]) = make_uint4(0, 0, 0, 0);
    if (tid < n_du) *reinterpret_cast<uint4 *>(&tile[tid][64]) = make_uint4((uint32_t)(uint16_t)PJD_COEF_SENTINEL, 0, 0, 0);
    // Tables of the range, no division per unit: component of every unit; whether it is the first unit of an MCU that starts a
    // restart segment (the DC stage resets the predictors there); the grid position of every MCU
    if (tid < PJD_IDCT_MAX_DU) {
        const uint32_t ml = pjd_div_small(tid, c_recip16[dus]), kk = tid - __umul24(ml, dus);   // the range starts on an MCU boundary
        comp_of[tid] = (uint8_t)(kk < nl ? 0 : kk - nl + 1);
        if (kk != 0) du_head[tid] = 0;                          // the entries of first units come from the MCU's thread
    }
    if (tid < wg.n_mcu) {                                       // the only divisions: one per MCU, none per unit
        const uint32_t m = wg.first_mcu + tid, my = m / im.mcux;
        mcu_xy[tid] = (my << 16) | (m - my * im.mcux);
        du_head[__umul24(tid, dus)] = (uint8_t)(m == im.first_mcu || (RI != 0 && m % RI == 0));
    }

    // units of this range that were decoded: all, unless the picture's first entropy-coding error lies in or before the range (the
    // others keep zero coefficients, as in the reference, whose buffers start zeroed and which stops at the error)
    const unsigned long long err_key = B.imstate[wg.image].err_key;
    const uint32_t n_valid = pjd_units_decoded(err_key, wg.first_mcu * dus, n_du);
    const uint32_t err_byte = (uint32_t)(err_key >> 35);       // byte of the stream the offending symbol starts in (bit positions fit 32 bits); no error: past every lane
    const PjdDevMark mark = B.marks[iwg];
    const uint32_t lane_end = im.lane_base + im.n_lane;
    uint32_t q = mark.lane, n = mark.ent_off;
    (void)n;
    if (n_valid == 0) { q = im.lane_base; n = 0; }              // nothing to parse: the mark may never have been written
    else if (q < im.lane_base || q >= lane_end) return;         // never on a verified image; keeps a stale mark harmless
    // predictors at the first unit: lane start (block-relative or absolute) + block carry + sums inside the lane
    uint32_t pred0[3];
    {
        const PjdDevLaneDc ld = B.lane_dc[q];
        const uint16_t *carry = B.dc_blk + (size_t)(q / PJD_DC_BLOCK) * 8 + 4;
#pragma unroll
        for (int c = 0; c < 3; c++) pred0[c] = (uint32_t)ld.dc_in[c] + (ld.abs ? 0u : (uint32_t)carry[c]) + mark.acc[c];
    }
    __syncthreads();
    // ---- parse: entries -> tile, one thread per GROUP (32 bytes: a head and 14 entries, pjd_internal.h) of a lane.  The write pass
    // left in every head where the group's first entry stands (units completed in the lane before it, slot it fills from) and with
    // every lane the unit its first entry belongs to (PjdDevLaneInfo::first_du), so a thread walks its 14 entries on its own: a DC
    // entry opens a unit, an AC entry lands on slot + run, the LAST bit closes the unit -- no scans over entries, no barriers
    // between chunks (round 2: two wave scans and two barriers per 1024 entries, ~70 instructions per entry against ~25 here).
    // Lanes are taken in windows of 32 (a range of 96 units spans 3-4 lanes of a dense picture, ~20 of 128 bytes); the window's
    // table holds the groups before each lane, its first unit relative to the range and its entry count.
    {
        // ltab: [0..31] groups before lane i of the window, [32..63] first_du - U0, [64..95] entries
        const uint32_t U0 = wg.first_mcu * dus;
        const uint32_t tile_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int16_t *)&tile[0][0];
        const uint32_t g0 = mark.ent_off / PJD_GROUP;          // the range starts in this group of lane q
        // where the NEXT range starts (its mark) bounds this one; usable when every unit of this range was decoded
        uint32_t q_end = 0xffffffffu, g_end = 0;
        if (n_valid == n_du && iwg + 1 < im.iwg_base + im.n_iwg) {
            const PjdDevMark nm = B.marks[iwg + 1];
            if (nm.lane >= q && nm.lane < lane_end) { q_end = nm.lane; g_end = nm.ent_off / PJD_GROUP; }
        }
        for (uint32_t qw = q; n_valid != 0; qw += 32) {
            bool more = false;
            if (tid < 32) {
                const uint32_t ql = qw + tid;
                uint32_t ng = 0, fd = 0, ne = 0;
                if (ql < lane_end) {
                    const PjdDevLaneInfo li = B.lane_info[ql];
                    fd = (li.first_du & 0x0fffffffu) - U0;                  // "negative" for the lane the range starts in
                    ne = li.n_ent;
                    // a lane that starts BEHIND the picture's first entropy-coding error holds what the reference never decoded; when the
                    // erring unit was still open at the error (an error in its AC part), that lane's leading entries would land in it
                    const bool in = (ql == q || (int)fd < (int)n_valid) && (ql == q || B.lanes[ql].byte_start <= err_byte);
                    if (in && ql <= q_end) {
                        const uint32_t gs = ql == q ? g0 : 0u, all = (ne + PJD_GROUP - 1) / PJD_GROUP;
                        uint32_t ge = ql == q_end ? (g_end + 1 < all ? g_end + 1 : all) : all;
                        ng = ge > gs ? ge - gs : 0u;
                    }
                    more = in && ql < q_end;
                }
                uint32_t inc = ng;
#pragma unroll
                for (int off = 1; off < 32; off <<= 1) { const uint32_t t = __shfl_up(inc, off); if ((int)tid >= off) inc += t; }
                ltab[tid] = inc - ng; ltab[32 + tid] = fd; ltab[64 + tid] = ne;
                if (tid == 31) { wagg[0] = inc; wagg[1] = more ? 1u : 0u; }   // groups in the window; the lane behind it may belong to the range too
            }
            __syncthreads();
            const uint32_t G = wagg[0];
            const bool again = wagg[1] != 0 && qw + 32 < lane_end;
            for (uint32_t w = tid; w < G; w += PJD_IDCT_THREADS) {
                uint32_t li_ = 0;                                           // last lane of the window whose groups start at or before w
#pragma unroll
                for (uint32_t step = 16; step != 0; step >>= 1) if (ltab[li_ + step] <= w) li_ += step;
                const uint32_t ql = qw + li_;
                const uint32_t g = w - ltab[li_] + (ql == q ? g0 : 0u);
                const uint32_t ne = ltab[64 + li_];
                const uint32_t cnt = ne - g * PJD_GROUP < PJD_GROUP ? ne - g * PJD_GROUP : PJD_GROUP;      // slots of this group that are in use (even)
                const uint4 *src = reinterpret_cast<const uint4 *>(B.ent + im.ent_base + (size_t)(ql - im.lane_base) * im.lane_cap + (size_t)g * PJD_GROUP);
                const uint4 r0 = src[0], r1 = src[1];                       // the group: 32 bytes, 32-byte aligned
                const uint32_t wds[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                const uint32_t head = wds[0];
                uint32_t u = ltab[32 + li_] + (head >> 8);                  // unit of the group's first entry, relative to the range ("negative" before it)
                uint32_t slot = head & 63u;                                 // 0: that entry is a DC difference; else the next free zigzag slot of the open unit
#pragma unroll
                for (int k = 1; k < PJD_GROUP / 2; k++) {                   // the group's step words: entry A, and entry B unless it is PJD_ENT_NONE
                    const uint32_t sw = wds[k];
                    const bool on = (uint32_t)(2 * k) < cnt;
                    {   // A: ONE path for both kinds of entry (the lanes of a wave stand at DC and AC entries at once): a DC difference
                        // (slot == 0) is an entry with "run + 1" = 1 that lands on position 0 and is DEQUANTISED like any other: the DC
                        // stage then sums products instead of multiplying the sum -- the same number modulo 2^16, which is all the
                        // reference keeps (src/jpeg_scanner.cpp:485-486 stores the predictor as a short, src/decoder_dpu.c:169-172 the product)
                        const bool dc = slot == 0;
                        const uint32_t f = dc ? 1u : sw & 31u;              // run + 1; 0: EOB
                        const uint32_t ns = slot + f, pos = ns - 1u;        // an EOB gives slot - 1: stores nothing (below)
                        if (on && f != 0 && pos < 64 && u < n_valid && PJD_LANES_KEEP(u)) {
                            const int val = dc ? (int)(int16_t)(sw & 0xffffu) : (int)(sw << 16) >> 21;
                            const uint32_t qe = qz[comp_of[u]][pos];        // (slot 52 under the quirk: position 64, quantiser 1)
                            // the low 16 bits of value x quantiser (reference src/decoder_dpu.c:169-172) depend on the low 16 bits of both only
                            pjd_tile_put(tile_lds, u, qe >> 16, pjd_mul_u24((uint32_t)val, qe));
                        }
                        if (on) {
                            const bool last = f == 0 || ns > 63;            // EOB, or the entry landed on slot 63 (or past it: a broken stream)
                            slot = last ? 0u : ns;
                            u += last ? 1u : 0u;
                        }
                    }
                    {   // B: the second symbol of a pair -- an AC entry of the unit A left open
                        const uint32_t f = (sw >> 16) & 31u;
                        const bool onb = on && f <= 16;                     // PJD_ENT_NONE: "run + 1" = 31
                        const uint32_t pos = slot + f - 1u;
                        if (onb && f != 0 && pos < 64 && u < n_valid && PJD_LANES_KEEP(u)) {
                            const int val = (int)sw >> 21;
                            const uint32_t qe = qz[comp_of[u]][pos];
                            pjd_tile_put(tile_lds, u, qe >> 16, pjd_mul_u24((uint32_t)val, qe));
                        }
                        if (onb) {
                            const uint32_t ns = slot + f;
                            const bool last = f == 0 || ns > 63;
                            slot = last ? 0u : ns;
                            u += last ? 1u : 0u;
                        }
                    }
                }
            }
            __syncthreads();
            if (!again) break;
        }
    }
#undef PJD_LANES_KEEP
