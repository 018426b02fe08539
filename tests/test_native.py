"""Host-side native pieces under the sanitizers (CPU only): the staging copy workers of
klf_stage (klogs_amd/csrc/klf_copypool.hpp) stressed from 8 caller threads under TSAN."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_copypool_tsan(tmp_path):
    exe = tmp_path / "cps"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-pthread",
                    str(ROOT / "tests" / "native" / "copypool_stress.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]
    assert "copypool: ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pattern_compiler_asan_ubsan(tmp_path):
    """klf_patterns.cpp alone with a small main (tests/native/patterns_fuzz.cpp) under ASan and
    UBSan: generated patterns and the position-limit patterns through compile_regex,
    regex_factors, compile_set, glushkov_match, prefilter_match at every phase and nfa_window;
    every decision equals the reference, refusals are KLF_ETOOBIG only, no sanitizer report."""
    import random
    import struct
    import sys
    sys.path.insert(0, str(ROOT / "tests"))
    import c_oracle as co
    import klf_oracle as po
    import rxfuzz
    exe = tmp_path / "pfz"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-pthread",
                    str(ROOT / "klogs_amd" / "csrc" / "klf_patterns.cpp"),
                    str(ROOT / "tests" / "native" / "patterns_fuzz.cpp"), "-o", str(exe)], check=True)
    rng = random.Random(5)
    recs = []
    for _ in range(150):
        p = rxfuzz.pattern(rng)
        recs.append((p.pattern, [rxfuzz.content(rng, [p]) for _ in range(8)]))
    runs = [b"", b"a" * 32, b"a" * 33, b"a" * 64, b"a" * 66, b"abcdefgh" * 8, b"abcdefgh" * 7]
    for lim in (rb"a{64}", rb"a{65}", rb"(?:a{1,}){32}", rb"(?:a{1,}){33}", rb"(?:abcdefgh{1,}){8}", rb"(?:abcdefgh+){8}",
                rb"(?:abcdefgh+){9}", rb"(?:a{2,3}){21}", rb"(?:a{2,3}){22}"):
        recs.append((lim, runs))
    blob = b"".join(struct.pack("<I", len(p)) + p + struct.pack("<I", len(cs))
                    + b"".join(struct.pack("<I", len(c)) + c for c in cs) for p, cs in recs)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(recs)] == "patterns_fuzz: ok"
    n_big = n_win = 0
    for k, ((pat, cs), line) in enumerate(zip(recs, lines)):
        assert line != "bad", pat
        if line == "big":
            n_big += 1
            continue
        # Python re is the reference, the C leg the second; the position-limit patterns (nested
        # repetitions of one byte: exponential backtracking in re) have the linear-time C leg alone
        ref = po.Pattern("regex", pat) if k < 150 else None
        for c, bits in zip(cs, line.split()):
            want = co.rx_match(pat, c)
            if ref is not None:
                assert ref.matches(c) is want, (pat, c)
            want = "1" if want else "0"
            assert len(bits) == 18 and bits[:17] == want * 17, (pat, c, bits)
            # the windows of every factor position together cover every match start
            assert bits[17] in (want, "x"), (pat, c, bits)
            n_win += bits[17] != "x"
    assert n_win >= 1000, n_win
    assert 3 <= n_big <= 3 + 15, n_big  # a{65}, (?:abcdefgh+){9}, (?:a{2,3}){22}; at most 10 % of the generated
