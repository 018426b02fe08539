"""The input stream seams of tests/seams.py on the host: the layouts are klf_layout's, the
two oracles agree on every stream, and every seam is hostile -- an oracle that reads 64
bytes past the stream's end answers differently.  That is what keeps tests/test_gpu_seams.py
from passing vacuously: a kernel that trusts the bytes behind a stream fails there.  No GPU."""
import pytest

import c_oracle as co
import klf_oracle as po
import seams
from klogs_amd import engine as E
from klogs_amd import synth

S = seams.build()
LAYOUTS = {"A": S.A, "B": S.B}
GZ = po.GO_ZERO_TIME


def test_text_size():
    assert (1 << 20) <= len(S.T) <= (3 << 19)
    assert S.T.endswith(b"\n") and S.T == seams.build.__wrapped__(20241022).T  # seeded


@pytest.mark.parametrize("name", ["A", "B"])
def test_layout_is_klf_layout(name):
    lay = LAYOUTS[name]
    bases, total = E.layout(lay.lens)
    assert bases.tolist() == lay.bases
    assert total == len(lay.buf) and E.layout([1])[1] == seams.ALIGN + seams.SLACK
    off = S.T.find(lay.buf[:4096])
    assert S.T[off:off + len(lay.buf)] == lay.buf  # contiguous T, through pads and slack
    for i, s in enumerate(lay.seams):
        assert s.stream == i and s.cut == lay.bases[i] + lay.lens[i]
    if name == "A":
        assert all(b % seams.ALIGN == 0 and n % seams.ALIGN == 0 and n > 0 for b, n in zip(lay.bases, lay.lens))
        assert all(lay.bases[i] + lay.lens[i] == lay.bases[i + 1] for i in range(len(lay.lens) - 1))  # they touch
    else:
        gaps = [lay.bases[i + 1] - lay.bases[i] - lay.lens[i] for i in range(len(lay.lens) - 1) if lay.lens[i]]
        assert all(1 <= g <= 255 for g in gaps) and {1, 255} <= set(gaps)
        assert [n for n in lay.lens if n < 64] == list(seams.TINY)


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_class_has_its_seams(name):
    lay = LAYOUTS[name]
    ks = {}
    for s in lay.seams:
        ks.setdefault(s.cls, []).append(s.k)
    nd = seams.set_needles()
    assert ks["prefix_cut"] == list(range(1, 32))
    assert ks["needle_cut"] == list(range(1, len(synth.NEEDLE)))
    for k, v in nd.items():
        assert ks[k + "_cut"] == [j for n in v for j in range(1, len(n))]
    assert sorted(len(n) for v in nd.values() for n in v)[:7] == [4, 5, 6, 7, 8, 9, 12]
    assert ks["anch_cut"] == list(range(1, len(seams.anchored_needle())))
    assert ks["rx_c5_cut"] == list(range(1, len(synth.c5_pattern(27, 1))))
    for c in ("noncanon_zone", "noncanon_frac12", "noncanon_hour1", "noncanon_comma"):
        assert len(ks[c]) >= 5
    for c in ("clean_after_nl", "cut_before_nl", "rx_fold_cut", "rx_took_cut", "rx_left_half", "rx_unbounded", "long_line", "dense_tail"):
        assert len(ks[c]) >= 2
    if name == "B":
        assert ks["tiny"] == list(seams.TINY)
    for c in ks:  # each class on a tile boundary and off it (the tiny streams have no tile to fill)
        if c != "tiny":
            assert {s.tile_aligned for s in lay.seams if s.cls == c} == {True, False}, c
    for s in lay.seams:
        span = lay.lens[s.stream] if name == "A" else -(-lay.lens[s.stream] // seams.ALIGN) * seams.ALIGN
        assert s.tile_aligned == (span % seams.TILE == 0)
    tiles, on_group = 0, []
    for i, n in enumerate(lay.lens):  # the engine numbers the batch's tiles stream after stream
        tiles += -(-n // seams.TILE)
        if n and tiles % seams.GROUP_TILES == 0:
            on_group.append(i)
    assert on_group and all(lay.seams[i].group for i in on_group)
    assert any(n > 65536 for n in lay.lens)
    for s in lay.seams:  # the dense tails: over one line start per 32 bytes in the stream's last tile
        if s.cls == "dense_tail":
            last = lay.stream(s.stream)[(lay.lens[s.stream] - 1) // seams.TILE * seams.TILE:]
            assert last.count(b"\n") > len(last) // 32 and (last.count(b"\n") > 1000 or not s.tile_aligned)


def test_pattern_sets_take_their_paths(monkeypatch):
    sets = seams.pattern_sets()
    for name, stride in (("lit2", 2), ("lit4", 4), ("lit6", 6), ("lit8", 8)):
        info = E.debug_prefilter(b"", grep=sets[name][0])[1]
        assert info["on"] and info["stride"] == stride and info["anchor"] is None, (name, info)
    assert not E.debug_prefilter(b"", grep=sets["off"][0], match=sets["off"][1])[1]["on"]
    assert E.debug_prefilter(b"", match=sets["rx"][1])[1]["on"]
    monkeypatch.setenv("KLF_QF_ANCHOR", "force")
    info = E.debug_prefilter(b"", grep=sets["anch"][0])[1]
    assert info["stride"] == 8 and info["anchor"] is not None, info


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("sname", ["none", "needle", "lit2", "lit4", "lit6", "lit8", "anch", "rx", "mixed", "off"])
def test_c_and_python_oracles_agree(name, sname):
    lay = LAYOUTS[name]
    grep, match = seams.pattern_sets()[sname]
    pats = po.compile_patterns(grep, match)
    # (a set with a regex: its literals hold no metacharacter and go to the C leg as regexes)
    assert not match or all(g.replace(b"_", b"").isalnum() for g in grep)
    rs = co.RegexSet(list(grep) + list(match)) if match else None
    for since, tail in ((None, -1), (lay.mid, 3)):
        for i, s in enumerate(lay.streams()):
            ref = po.filter_stream(s, since or GZ, tail, pats)
            if rs:  # the C leg's own restatement of Go regexp
                out, lo, bits, c = co.filter_stream_rx(s, since or GZ, tail, rs)
            else:   # (seams.expected: the C oracle, as the GPU tests use it)
                w = seams.expected(name, sname, since, tail)[i]
                out, lo, bits, c = w["out"], w["lines"], w["bits"], w["counts"]
            assert out == ref.out and list(lo) == ref.line_off, (since, tail, i)
            assert bits == ref.match_bits, (since, tail, i)
            assert [c[k] for k in seams.COUNT_KEYS] == \
                [ref.n_lines, ref.n_parsed, ref.n_since, ref.n_matched, ref.n_selected, len(ref.out)], (since, tail, i)


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_seam_is_hostile(name):
    """Condition, not measurement: each seam's `expect` names the pattern set and the field
    that must change when the oracle is given the 64 bytes behind the stream as well (the
    parsed count where the neighbour completes a prefix, the matched count and the match
    bits where it completes a needle or a regex match, the line count where it adds a
    newline, the output where the cut line matches on its own and only grows).  Only the
    clean cut after a newline is exempt."""
    lay = LAYOUTS[name]
    assert sum(s.control for s in lay.seams) == lay.classes()["clean_after_nl"]
    for s in lay.seams:
        if s.control:
            assert s.cls == "clean_after_nl" and lay.stream(s.stream).endswith(b"\n")
            continue
        sname, key = s.expect
        exact = seams.expected(name, sname)[s.stream]
        over = seams.oracle(lay.stream(s.stream, seams.OVER), sname)
        tag = (s.cls, s.k, s.stream)
        if key == "out":
            assert over["out"] != exact["out"], tag
        else:
            assert over["counts"][key] != exact["counts"][key], (tag, exact["counts"], over["counts"])
        if key == "matched":
            assert over["bits"] != exact["bits"], tag
            assert over["counts"]["matched"] == exact["counts"]["matched"] + 1, tag


def test_staged_buffer_keeps_every_seam_hostile():
    """The staged and follow legs of test_gpu_seams run one batch (seams.staged_first) and then
    every piece of both layouts on the same engine.  Simulated here: the second batch fits the
    first one's buffer, klf_layout puts layout B's pieces where they lay in the first batch and
    layout A's behind them, and behind every seam of both layouts the buffer still holds the
    completion -- the same condition as test_every_seam_is_hostile, on the staged bytes."""
    buf, bases, lens = seams.staged_buffer()
    first = seams.staged_first()
    assert first.endswith(b"\n") and buf[:len(first)] == first  # the pieces land on their own bytes
    got, total = E.layout(lens)
    assert got.tolist() == bases and total <= E.layout([len(first)])[1] == len(buf)
    assert bases[:len(S.B.lens)] == S.B.bases and lens == S.B.lens + S.A.lens
    n = 0
    for name, off in (("B", 0), ("A", len(S.B.lens))):
        for s in LAYOUTS[name].seams:
            if s.control:
                continue
            i = off + s.stream
            assert buf[bases[i]:bases[i] + lens[i]] == LAYOUTS[name].stream(s.stream)
            sname, key = s.expect
            exact = seams.expected(name, sname)[s.stream]
            over = seams.oracle(buf[bases[i]:bases[i] + lens[i] + seams.OVER], sname)
            tag = (name, s.cls, s.k, s.stream)
            if key == "out":
                assert over["out"] != exact["out"], tag
            else:
                assert over["counts"][key] != exact["counts"][key], (tag, exact["counts"], over["counts"])
            n += 1
    assert n == sum(not s.control for lay in LAYOUTS.values() for s in lay.seams)
