"""GPU (-m gpu): hdlz_png_index_ws and hdlz_png_decode_ws under HDLZ_PNG_ADAM7 inside guard bands (tests/guards.py).  The guarded calls
are those of tests/test_gpu_png_containment.py (index_call, decode_call), run with the rule of tests/png_adam7_ref.py in the place of
png_ref's index: a mixed batch -- every interlaced geometry of 1 .. 9 x 1 .. 9, one 140 x 70 RGBA 16 image, plain and damaged files --
must leave every band, every read-only region and every byte outside the records, the slots' out_len bytes and the scratch it was given
as they were, and give the same results on the pattern and on its complement."""
import pytest

import png_ref as P
import png_adam7_ref as A
import test_gpu_png_adam7 as G
import test_gpu_png_containment as C

pytestmark = pytest.mark.gpu


def _batch(flags):
    items = [G.made(w, h, *((2, 8) if (w + h) % 3 else (0, 1)), seed=10 * w + h, flags=flags) for w in range(1, 10) for h in range(1, 10)]
    items.append(G.made(140, 70, 6, 16, seed=3, flags=flags, level=1))
    for k in range(3):                                          # plain files between them
        rows = P.random_rows(11 + k, 6, *P.PAIRS[4 * k], k)
        f = P.make_png(11 + k, 6, *P.PAIRS[4 * k], rows=rows, filters=[r % 5 for r in range(6)], seed=k)
        rec = P.index([f], flags & P.EXPAND)["images"][0]
        items.insert(20 * k + 5, (f, (P.OK, P.expand(rows, rec, f) if flags & P.EXPAND else rows)))
    broken = [items[30][0][:-15], P.make_png(9, 9, 2, 8, interlace=2)]
    short = bytearray(items[50][0])
    short[-14] ^= 1                                             # the last IDAT's CRC
    for k, f in enumerate(broken + [bytes(short)]):
        items.insert(17 * k + 9, (f, None))
    files = [f for f, _ in items]
    ix = A.index(files, flags)
    expect = [e if e is not None else A.decode(f, rec, flags) for (f, e), rec in zip(items, ix["images"])]
    assert sorted({s for s, _ in expect}) == sorted({P.OK, P.E_NO_EOF, P.E_BAD_HEADER, P.E_BAD_CHECKSUM})
    return files, expect


def test_the_index_stays_inside_its_records_with_the_flag(engine, monkeypatch):
    monkeypatch.setattr(P, "index", A.index)
    files, _ = _batch(G.EX)
    n = len(files)
    C.index_call(engine, "mixed, exact", files, G.EX, 64, n)
    C.index_call(engine, "mixed, apart, at an odd address, raw", files, G.RAW, 1, n, gap=37, mis=3)
    C.index_call(engine, "mixed, room for 5", files, G.EX, 16, 5, mis=1)
    C.index_call(engine, "mixed, the sizing call", files, G.RAW, 64, 0)


@pytest.mark.parametrize("flags", [G.EX, G.RAW], ids=["expand", "raw"])
def test_the_decode_stays_inside_the_slots_with_the_flag(engine, monkeypatch, flags):
    monkeypatch.setattr(P, "index", A.index)
    files, expect = _batch(flags)
    n = len(files)
    C.decode_call(engine, ("mixed", flags), files, expect, flags, 0, n, mis=3, out_mis=1 if flags == G.RAW else 0)
    C.decode_call(engine, ("mixed, apart, packed slots", flags), files, expect, flags, 0, n, gap=11, mis=5, slack=100, out_align=1, out_mis=3)
    C.decode_call(engine, ("a sub-range", flags), files, expect, flags, 7, 40, gap=2)
    big = next(k for k, f in enumerate(files) if len(f) > 20000)
    for e in (0, 5, 9, big):                                    # interlaced, plain, broken, the 140 x 70 image: alone in a call
        C.decode_call(engine, ("alone", e, flags), files, expect, flags, e, 1, mis=e % 7)
