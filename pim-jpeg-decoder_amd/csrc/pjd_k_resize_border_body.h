// pjd_k_resize_border_body.h -- the body of pjd_k_resize_border (pjd_k_resize.hip): one wave, one line of one padded canvas.  A textual
// include for one reason: tools/resize_host.cpp runs this very text on the host, thread by thread (no lane reads another's registers).
// A line is a row of an interleaved canvas (3 * W elements) or a row of one plane of a planar one (W elements); its runs of fill are
// [0, end) where the row lies in the top or bottom band, [0, left) and [left + cw, W) otherwise, in pixels.  Per run: the bytes up to
// the first 4-byte aligned ADDRESS one by one, then dwords -- lane l the dwords l, l + 64, ... -- then the bytes behind the last whole
// dword.  The dword at byte j of the line is pjd_pad_fill_dword(.., j): the alignment of the address says nothing about j.
// In scope: lane, line (uniform), dst, recs, pad, line_prefix, n_images, n_lines, planar, es (bytes per element), fill.
    if (line >= n_lines) return;
    uint32_t lo = 0, hi = n_images;
    while (hi - lo > 1) {                                  // the last picture whose prefix is <= line: pictures without lines are passed over
        const uint32_t mid = (lo + hi) >> 1;
        if (line_prefix[mid] <= line) lo = mid; else hi = mid;
    }
    const PjdDevResizePad cv = pad[lo];
    const uint32_t l = line - line_prefix[lo];
    const uint32_t c = planar ? l / cv.H : 0u, y = planar ? l - c * cv.H : l;
    const uint32_t px = planar ? es : 3u * es;             // bytes per pixel of a line
    const uint32_t p0 = fill.d[planar ? c : 0u], p1 = fill.d[planar ? c : 1u], p2 = fill.d[planar ? c : 2u];
    uint8_t *const lp = dst + recs[lo].dst_off + ((uint64_t)c * cv.H + y) * cv.W * px;
    const bool band = y < cv.top || y >= cv.top + cv.ch;
    // the two runs, in bytes of the line (the second one empty in a band)
    const uint32_t run_a[2] = {0u, band ? 0u : (cv.left + cv.cw) * px};
    const uint32_t run_b[2] = {band ? cv.W * px : cv.left * px, band ? 0u : cv.W * px};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t a = run_a[k], n = run_b[k] - a;
        if (n == 0u) continue;                             // uniform
        uint8_t *const p = lp + a;
        const uint32_t mis = (uint32_t)(0u - (uintptr_t)p) & 3u, head = mis < n ? mis : n;
        const uint32_t nd = (n - head) >> 2, tail0 = head + 4u * nd;
        if (lane < head) p[lane] = (uint8_t)pjd_pad_fill_dword(p0, p1, p2, a + lane);
        for (uint32_t d = lane; d < nd; d += 64u)
            *reinterpret_cast<uint32_t *>(p + head + 4u * d) = pjd_pad_fill_dword(p0, p1, p2, a + head + 4u * d);
        if (lane < n - tail0) p[tail0 + lane] = (uint8_t)pjd_pad_fill_dword(p0, p1, p2, a + tail0 + lane);
    }
