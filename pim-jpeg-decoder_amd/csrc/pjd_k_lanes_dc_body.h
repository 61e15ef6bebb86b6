// pjd_k_lanes_dc_body.h -- DC prediction over one back-end range by wave 0 (lane = tid & 63), included textually behind
// pjd_k_lanes_parse_body.h: the differences the parser left in tile[u][0] become absolute values, scaled by the quantisers in qz.
        // the parser left DEQUANTISED differences: the predictors that enter the range are scaled the same way (all modulo 2^16)
        const uint32_t q0y = qz[0][0] & 0xffffu, q0b = qz[1][0] & 0xffffu, q0r = qz[2][0] & 0xffffu;
        uint32_t cy = (pred0[0] * q0y) & 0xffffu, cc = ((pred0[1] * q0b) & 0xffffu) | ((pred0[2] * q0r) << 16);   // predictors entering the next group of 64 units
        for (uint32_t base = 0; base < n_du; base += 64) {
            const uint32_t u = base + lane;
            const bool on = u < n_valid;                        // an undecoded unit keeps DC 0: it is never predicted
            const uint32_t us = on ? u : 0u, comp = comp_of[us];
            const uint32_t dv = on ? (uint32_t)(uint16_t)tile[us][0] : 0u;             // the unit's DC difference as the parser left it (zero if the unit has none)
            const bool head = on && du_head[us] != 0;
            // sums since the group start (inclusive), Y | Cb, Cr packed; then the same sums at the last head at or before the unit
            uint32_t vy = comp == 0 ? dv : 0u, vc = comp == 1 ? dv : (comp == 2 ? dv << 16 : 0u);
            PJD_WAVE_SCAN(pjd_op_add, vy);
            PJD_WAVE_SCAN(pjd_op_pkadd, vc);
            uint32_t hpos = head ? lane + 1 : 0u;               // 1 + lane of the last head at or before this unit
            PJD_WAVE_SCAN(pjd_op_max, hpos);
            // a head resets the predictors BEFORE its own difference is added: subtract the sums just before it
            const uint32_t hl = hpos ? hpos - 1 : 0u;           // lane of that head
            const uint32_t by = __shfl(vy, (int)hl) - __shfl(comp == 0 ? dv : 0u, (int)hl);
            const uint32_t bc = __shfl(vc, (int)hl), bc_own = __shfl(comp == 1 ? dv : (comp == 2 ? dv << 16 : 0u), (int)hl);
            uint32_t ty = vy, tc = vc;
            if (hpos) { ty -= by; tc = pjd_op_pksub(tc, pjd_op_pksub(bc, bc_own)); }
            else { ty += cy; tc = pjd_op_pkadd(tc, cc); }
            if (on) {
                const uint32_t dcv = comp == 0 ? ty : (comp == 1 ? tc : tc >> 16);
                tile[u][0] = (int16_t)dcv;
            }
            cy = __shfl(ty, 63); cc = __shfl(tc, 63);
        }
