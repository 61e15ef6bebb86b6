// pjd_k_dense_stage_body.h -- dense staging of one lane: the scratch the exact kernel and the progressive scans fill holds a unit in
// zigzag-slot order with absolute DC values; the lane takes the 16 bytes `raw` (int4) of slots 8r..8r+7 of unit `du` and scatters them
// to natural order into tile[du].  Included textually inside the caller's loop -- all units of the range, or its luma units alone --
// for the reason pjd_k_idct_dense_body.h gives (as functions the two texts moved instructions in every kernel that uses them:
// profiles/backend_shared_stages.md).  Uses tile, du, r, raw and im of the including loop.  Two texts:
//   default            dequantising, for the reference's arithmetic (pjd_k_idct_colour<*>, pjd_k_idct_colour_planar<*>, pjd_k_idct_gray<*>);
//                      PJD_DENSE_Q of the includer is the unit's quantiser by natural position
//   PJD_DENSE_RAW      as decoded, for PJD_F_LIBJPEG pictures, whose IDCT multiplies by the quantiser itself (pjd_k_idct_std_dense,
//                      pjd_k_idct_gray_std_dense); `sentinel` of the including kernel is !(im.flags & PJD_IF_PROGRESSIVE), taken once
// The two rules of the scratch live here and nowhere else:
//   the sentinel       PJD_COEF_SENTINEL means "explicit zero" at slot 52 of a baseline picture only; everywhere else -32768 is a value
//                      (an absolute DC the int16 predictor reached, a progressive coefficient shifted by Al)
//   slots 48 and 52    without PJD_IF_STANDARD_ZIGZAG natural position 38 is the target of slot 48 AND slot 52 (the reference's
//                      zigzag_map[48] = 38): the later write wins, and an explicit zero written at slot 52 (run/size symbol with size
//                      0) is marked by the sentinel; natural 58 is never written by the reference.  With the flag, and always under
//                      PJD_F_LIBJPEG, the zigzag is T.81's: slot 48 -> 58.
        const int16_t *rv = reinterpret_cast<const int16_t *>(&raw);
#ifdef PJD_DENSE_RAW
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t nat = (r == 6 && j == 0) ? 58u : c_zz[r * 8 + j];
            const bool zero52 = sentinel && r == 6 && j == 4 && rv[j] == PJD_COEF_SENTINEL;
            tile[du][nat] = zero52 ? (int16_t)0 : rv[j];
        }
#else
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = rv[j];
        int16_t *t = tile[du];
        const uint16_t *q = PJD_DENSE_Q;
        const bool zero52 = r == 6 && !(im.flags & PJD_IF_PROGRESSIVE) && v[4] == PJD_COEF_SENTINEL;
        if (r == 6 && !(im.flags & PJD_IF_STANDARD_ZIGZAG)) {
            const int v52 = v[4];
            const int n38 = v52 != 0 ? (zero52 ? 0 : v52) : v[0];
            t[38] = (int16_t)pjd_dequant(n38, q[38]);
            t[59] = (int16_t)pjd_dequant(v[1], q[59]);
            t[52] = (int16_t)pjd_dequant(v[2], q[52]);
            t[45] = (int16_t)pjd_dequant(v[3], q[45]);
            t[31] = (int16_t)pjd_dequant(v[5], q[31]);
            t[39] = (int16_t)pjd_dequant(v[6], q[39]);
            t[46] = (int16_t)pjd_dequant(v[7], q[46]);
            t[58] = 0;
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t nat = (r == 6 && j == 0) ? 58u : c_zz[r * 8 + j];          // r == 6 here: PJD_IF_STANDARD_ZIGZAG
                t[nat] = (int16_t)pjd_dequant(j == 4 && zero52 ? 0 : v[j], q[nat]);
            }
        }
#endif
