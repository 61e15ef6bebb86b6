"""The cases of test_gpu_fallback.py that need caller-owned device memory, each run in a process of its own:

    python fallback_torch_cases.py mixed_planar | mixed_gray | shards_rgb8 | shards_gray

torch is loaded, and touches the device, before anything of pjd_amd, so that both use one HIP runtime (as nosync_torch_cases.py).
Prints "CASE OK <case>" at the end; a failed assertion ends the process with a traceback."""
import torch                                                      # first: see above

assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

import os                                                         # noqa: E402
import sys                                                        # noqa: E402

import numpy as np                                                # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pim-jpeg-decoder_amd", "python"))

import fallback_corpus as F                                       # noqa: E402
import pjd_amd                                                    # noqa: E402
import test_gpu_fallback as T                                     # noqa: E402

GUARD = 0xA5


def _open():
    for k, v in T.ENV.items():
        os.environ[k] = v
    for k in T.ENV_OFF:
        os.environ.pop(k, None)
    return pjd_amd.Context(0)


def _bound_decodes(ctx, descs, fmt, n_sequential, n_fallback, statuses, check):
    """The batch bound at base + 1 with an odd gap behind every picture in a tensor of GUARD bytes; decoded twice, captured and replayed.
    check(k, bytes of picture k) after every decode; every byte outside the pictures must still be GUARD."""
    with ctx.batch(descs, T.fmt_of(fmt)) as b:
        sizes = [b.output_size(i) for i in range(len(descs))]
        offsets, off = [], 1
        for i, n in enumerate(sizes):
            offsets.append(off)
            off += n + 3 + 2 * (i % 5)
        cap = off + 64
        buf = torch.full((cap,), GUARD, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert buf.data_ptr() % 2 == 0
        b.bind_output(buf.data_ptr(), cap, offsets)
        b.upload()
        used = np.zeros(cap, bool)
        for o, n in zip(offsets, sizes):
            used[o:o + n] = True
        seen = []
        for what in ("first", "second", "replay"):
            if what == "replay":
                b.capture()
            b.decode(); b.sync()
            assert b.statuses() == list(statuses), (what, b.statuses(), statuses)
            info = b.info()
            assert (info["n_sequential"], info["n_fallback"]) == (n_sequential, n_fallback), (what, info)
            assert (info["exact_fallback_ms"] > 0) == (n_fallback > 0), (what, info["exact_fallback_ms"])
            T.no_defensive_flag(info, what)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            guard = host[~used]
            assert (guard == GUARD).all(), (what, "guard bytes overwritten", int((guard != GUARD).sum()), np.flatnonzero(~used)[guard != GUARD][:8].tolist())
            for k, (o, n) in enumerate(zip(offsets, sizes)):
                check(what, k, host[o:o + n])
            seen.append(host.tobytes())
        assert seen[0] == seen[1] == seen[2]
    del buf


def _equal(got, want, label):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.size == want.size, (label, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, "first differing byte", int(bad[0]), "of", want.size, "differing", int(bad.size), got[bad[:4]].tolist())


def case_mixed(fmt):
    gray = fmt == "gray"
    items = list(T.mixed())
    exp = [T.expected(it, gray) for it in items]
    wants = [p if gray else np.ascontiguousarray(p.transpose(2, 0, 1)) for _, p in exp]
    sc = [T.scan(it) for it in items]
    ctx = _open()
    try:
        _bound_decodes(ctx, [x.desc for x in sc], fmt, sum(T.is_sequential(it) for it in items), T.MIXED_FALLING, [st for st, _ in exp],
                       lambda what, k, got: _equal(got, wants[k], (what, k, items[k].label)))
    finally:
        ctx.close()


def case_shards(fmt):
    """A batch of one shard each.  Rows [y0, y0 + rows) of the picture are the oracle's decode of the shard file; the rows above and
    below keep the guard byte, like the tensor around the picture."""
    gray = fmt == "gray"
    ctx = _open()
    n_fb = 0
    try:
        for sh in F.shards():
            sc = pjd_amd.Scanned(sh.data)
            assert sc.valid
            sc.desc.shard_first_seg, sc.desc.shard_n_segs = sh.r0, sh.r1 - sh.r0
            w, h = int(sc.desc.width), int(sc.desc.height)
            status, part = T.want(sh.file, False, 1, gray)
            y0, rows = sh.rows
            assert part.shape[:2] == (rows, w)
            ch = 1 if gray else 3
            whole = np.full((h, w * ch), GUARD, np.uint8)
            whole[y0:y0 + rows] = part.reshape(rows, w * ch)

            def check(what, k, got, whole=whole, sh=sh):
                _equal(got, whole, (what, sh.name))

            _bound_decodes(ctx, [sc.desc], fmt, 0, int(sh.holds_broken), [status], check)
            n_fb += sh.holds_broken
    finally:
        ctx.close()
    assert n_fb == 4


if __name__ == "__main__":
    kind, fmt = sys.argv[1].split("_")
    {"mixed": case_mixed, "shards": case_shards}[kind](fmt)
    print("CASE OK", sys.argv[1])
