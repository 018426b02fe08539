"""The reachable k_scan variants as a table of pattern sets and knobs (shared by
tests/test_prefilter.py, which checks the layouts on the host, and
tests/test_gpu_scan_variants.py, which runs every entry), and the input they scan.

The stride follows the shortest needle -- lengths 3, 4/5, 6/7, 8/9, 10/>=11 give strides 1,
2, 4, 6, 8 with 3- / 4-byte grams (stride_rule) -- and the bits per gram the number of
probed grams: up to kQfK2MaxGrams = 1536 needles x stride give 2 bits, more give 3, or at
stride 4 the two-level probe (k = 5).  The layouts are placed without data statistics
(KLF_QF_TUNE=0), where nothing but the set and the knobs below decides them; the two `tuned`
entries go through the first batch's statistics, where KLF_QF_QMAX pins the gram length that
the cost estimate would otherwise choose (they repeat two variants: 27 distinct ones).
KLF_QF_GRID6 is read once per process and cannot be part of a table run in one process;
nothing here needs it (stride 6 is the default for 8- and 9-byte needles).
"""
import random
from collections import namedtuple

TILE = 8192
K2_MAX = 1536  # kQfK2MaxGrams
TWO_LEVEL = 5  # kQfTwoLevel
ALNUM = b"abcdefghijklmnopqrstuvwxyz0123456789"
# the shortest needle that gives (stride, gram bytes)
LENGTH = {(1, 3): 3, (2, 3): 4, (2, 4): 5, (4, 3): 6, (4, 4): 7, (6, 3): 8, (6, 4): 9, (8, 3): 10, (8, 4): 11}

# grep: the set; env: knobs; mode: "plain" / "one_pass" / "lit" / "gen"; S, q, k, anchored: the layout
Variant = namedtuple("Variant", "name grep env mode S q k anchored")
SHORT = [b"ab_cd1", b"xy_z9w", b"qr_stu"]  # anchored at '_' (offset 2 <= len - 4)


def needles(n, length, seed):
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add(bytes(rng.choice(ALNUM) for _ in range(length)))
    return sorted(out)


def _gen(name, S, q, k, length=None, n=3, env=None, anchored=False, tuned=False):
    if k == 3:
        n = K2_MAX // S + 8
    grep = needles(n, length or LENGTH[S, q], 1000 * S + 10 * q + k)
    if S == 1 and k == 3:  # one 3-byte needle sets the stride (1,500 of them would hit every line)
        grep = grep[:1] + needles(n, 5, 77)
    e = {} if tuned else {"KLF_QF_TUNE": "0"}
    e.update(env or {})
    return Variant(name, (SHORT if anchored else []) + grep, e, "gen", S, q, k, anchored)


def _table():
    t = [Variant("plain", [], {"KLF_FUSE": "0"}, "plain", 0, 0, 0, False),
         Variant("one_pass", [], {}, "one_pass", 0, 0, 0, False),
         Variant("literal", [b"ERR_CONN_RESET"], {}, "lit", 0, 0, 0, False)]
    for q in (3, 4):
        t.append(_gen(f"two_level_q{q}", 4, q, TWO_LEVEL, env={"KLF_QF_TWO": "force"}))
        for S in (2, 4, 6, 8):
            for k in (2, 3):
                t.append(_gen(f"s{S}_q{q}_k{k}", S, q, k, env={"KLF_QF_TWO": "0"} if S == 4 else None))
        for k in (2, 3):
            t.append(_gen(f"anchored_q{q}_k{k}", 8, q, k, env={"KLF_QF_ANCHOR": "force"}, anchored=True))
    for k in (2, 3):
        t.append(_gen(f"s1_q3_k{k}", 1, 3, k))
    # through the first batch's statistics, with needles whose length alone gives 4-byte grams
    t.append(_gen("tuned_two_level_q3", 4, 3, TWO_LEVEL, length=7, n=400, env={"KLF_QF_QMAX": "3"}, tuned=True))
    t.append(_gen("tuned_s8_q3_k2", 8, 3, 2, length=11, env={"KLF_QF_QMAX": "3"}, tuned=True))
    return t


TABLE = _table()
LENS = (2 * TILE + 1000, 9 * TILE + 17, 0)  # a partial last tile, a tile group of 8 crossed, an empty stream
T0 = 1729555200  # 2024-10-22T00:00:00Z
SINCE = (T0 + 100, 0)


def _stream(total, seed, plant, dense_tile):
    """`total` bytes of kubelet lines, one per second from T0: the needles of `plant` in turn
    across tile seams and in the last line (which has no final newline when seed is odd);
    tile `dense_tile` (if any) holds 300 more line starts (2-byte lines without a timestamp)."""
    rng = random.Random(seed)
    out, sec, k, seams = bytearray(), 0, 0, 0

    def filler(n):
        return bytes(rng.choice(ALNUM + b"  __=:.") for _ in range(n))

    def line(content):
        nonlocal sec
        sec += 1
        return b"2024-10-22T00:%02d:%02d.%09dZ " % (sec // 60, sec % 60, rng.randrange(10 ** 9)) + content + b"\n"

    while total - len(out) > 400:
        o = len(out)
        to_seam = (o // TILE + 1) * TILE - o
        if o // TILE == dense_tile and to_seam > 700:
            out += b"x\n" * 300
            dense_tile = None
        elif 40 < to_seam < 250 and plant:  # this line spans the seam: a needle across it
            nd = plant[k % len(plant)]
            k += 1
            seams += 1
            out += line(filler(to_seam - 31 - len(nd) // 2) + nd + filler(rng.randint(0, 60)))
        else:
            out += line(filler(rng.randint(10, 200)))
    nd = plant[k % len(plant)] if plant else b""
    final_nl = seed % 2 == 0
    last = line(filler(total - len(out) - 31 - final_nl - len(nd) - 3) + nd + filler(3))
    out += last if final_nl else last[:-1]
    assert len(out) == total and dense_tile is None and (seams or not plant), (len(out), total, dense_tile, seams)
    return bytes(out)


def streams(v, dense=True):
    """The three streams of entry v, needles of its set planted; dense: one tile with more
    line starts than the slot list holds."""
    plant = ([v.grep[0], v.grep[-1]] + v.grep[1:2] * v.anchored) if v.grep else []
    return [_stream(LENS[0], 2, plant, None), _stream(LENS[1], 3, plant, 4 if dense else None), b""]
