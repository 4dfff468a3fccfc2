"""The state file (include/msom_state.h, DESIGN.md "State file") on the host: no GPU.

msom_amd.state (read_state / write_state) is written from the format text and never calls the library; state_io.c is the library's
reader.  The two are held to each other here, a third statement of the digest stands in this file, and corrupted files must be
refused by msom_state_check with MSOM_ERR_IO and a message, in the library and in a stand-alone sanitizer build of state_io.c
(driver/state_check.c: its own main, not loaded into Python).

tests/golden/state_32x32x3.msom pins format version 1.  It was written by
    PYTHONPATH=. python tests/test_state_host.py --make-golden
which is make_golden() below: write_state of psi, q, t, dt, previous, iter of the CPU oracle after 3 steps of
orc.double_gyre_params(32, 3) from orc.synthetic_psi(3, 32, 32).  The oracle does not hand out the dt limiter's `previous`: it is
what the step's second update returns, so the third step is also made call by call on a second oracle, which must end on the
stepped oracle's bits.
"""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from msom_amd import api
from msom_amd.state import StateFormatError, digest, read_state, write_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "state_32x32x3.msom")
CSRC = os.path.join(ROOT, "msom_amd", "csrc")
MSOM_ERR_IO = -2


def golden_content():
    import orc
    txt = orc.double_gyre_params(32, 3)
    a, b = (orc.Oracle(txt, smoother=orc.GS_RB, quiet=1) for _ in range(2))
    for o in (a, b):
        o.set(orc.PSI, orc.synthetic_psi(3, 32, 32))
        o.set_const()
        o.step()
        o.step()
    a.step()
    # b: the third step call by call (msqg run(): update, dtnext with no event ahead, advance dt / 2, update, advance dt)
    dt = b.update(orc.Q, orc.DQ, b.param("DT"))
    b.advance(orc.QPRED, orc.Q, orc.DQ, dt / 2)
    previous = b.update(orc.QPRED, orc.DQ, dt)
    b.advance(orc.Q, orc.Q, orc.DQ, dt)
    assert dt == a.dt and np.array_equal(a.get(orc.Q), b.get(orc.Q)) and np.array_equal(a.get(orc.PSI), b.get(orc.PSI))
    return dict(records={"psi": a.get(orc.PSI), "q": a.get(orc.Q)}, nx=32, ny=32, nl=3, params=txt, t=a.t, dt=a.dt, previous=previous, iter=a.iter)


def make_golden():
    write_state(GOLDEN, **golden_content())


# ------------------------------------------------------------------ the format, three ways

def sample(rng, nx=16, ny=8, nl=3):
    return {"psi": rng.standard_normal((nl, ny, nx)), "q": rng.standard_normal((nl, ny + 2, nx + 2)),
            "mgstats": np.array([1, 2.5e-4, 1e-5, 4.0]), "rd": rng.standard_normal((1, ny, nx))}


def write_sample(path, rng=None, **kw):
    rec = sample(rng or np.random.default_rng(1))
    write_state(path, rec, 16, 8, 3, params="N = 16\nNy = 8\nnl = 3\n", ring=("q",), t=0.75, dt=0.01, previous=0.0125, iter=42, **kw)
    return rec


def test_python_round_trip(tmp_path):
    p = tmp_path / "a.msom"
    rec = write_sample(p, stochastic=1, noise_mode=1, flag_topo=1)
    d = read_state(p)
    assert (d["version"], d["dialect"], d["nx"], d["ny"], d["nl"], d["nptr"]) == (1, 0, 16, 8, 3, 0)
    assert (d["stochastic"], d["noise_mode"], d["mode_pv_invert"], d["flag_topo"]) == (1, 1, 0, 1)
    assert d["params"] == "N = 16\nNy = 8\nnl = 3\n"
    assert (d["t"], d["dt"], d["previous"], d["tnext"], d["iter"]) == (0.75, 0.01, 0.0125, float("inf"), 42)
    assert list(d["records"]) == ["time", "psi", "q", "mgstats", "rd"] and d["ring"] == ["q"]
    for k, a in rec.items():
        assert d["records"][k].shape == a.shape and np.array_equal(d["records"][k], a), k
    # special values keep their bits
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, np.finfo(float).max])
    write_state(p, {"x": odd}, 2, 2, 1)
    assert np.array_equal(read_state(p)["records"]["x"].view(np.uint64), odd.view(np.uint64))


def digest_by_the_text(a):
    """D = sum_k mix64(bits(x_k) + 0x9E3779B97F4A7C15 (k + 1)) mod 2^64 in Python integers, straight from the issue text"""
    M = (1 << 64) - 1
    d = 0
    for k, bits in enumerate(np.ascontiguousarray(a, dtype="<f8").reshape(-1).view(np.uint64).tolist()):
        z = (bits + 0x9E3779B97F4A7C15 * (k + 1)) & M
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & M
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & M
        z ^= z >> 31
        d = (d + z) & M
    return d


def test_digest_three_ways(tmp_path):
    """the C checker accepts a file only if its own digest of a payload equals the header's: the header's is numpy's, and both equal
    the integer restatement; the digest depends on position"""
    rng = np.random.default_rng(2)
    p = tmp_path / "a.msom"
    for shape in ((1, 2, 2), (3, 8, 16), (2, 31, 5)):
        a = rng.standard_normal(shape)
        assert digest(a) == digest_by_the_text(a)
        write_state(p, {"psi": a}, shape[2], shape[1], shape[0])
        assert api.state_check(p) == 2
        assert read_state(p)["digests"]["psi"] == digest_by_the_text(a)
    a = rng.standard_normal((2, 8, 8))
    assert digest(a) != digest(a.transpose(0, 2, 1)) and digest(a) != digest(np.roll(a, 1, axis=2)) and digest(a) != digest(a[::-1])


@pytest.mark.parametrize("strict", [False, True])
def test_library_reads_a_python_file(tmp_path, strict):
    p = tmp_path / "a.msom"
    write_sample(p, mode_pv_invert=1)
    assert api.state_check(p, strict=strict) == 5
    i = api.state_info(p, strict=strict)
    assert (i["version"], i["dialect"], i["nx"], i["ny"], i["nl"], i["nptr"], i["nrecords"]) == (1, 0, 16, 8, 3, 0, 5)
    assert (i["stochastic"], i["noise_mode"], i["mode_pv_invert"], i["flag_topo"]) == (0, 0, 1, 0)
    assert (i["t"], i["dt"], i["iter"]) == (0.75, 0.01, 42)
    assert i["names"] == ["time", "psi", "q", "mgstats", "rd"]


# ------------------------------------------------------------------ corrupted files

def rec_offsets(b):
    """(header offset, payload offset, nbytes) per record, by the layout text"""
    plen = struct.unpack_from("<I", b, 52)[0]
    pos, out = 64 + plen + (-plen % 8), []
    for _ in range(struct.unpack_from("<I", b, 48)[0]):
        nbytes = struct.unpack_from("<Q", b, pos + 40)[0]
        out.append((pos, pos + 64, nbytes))
        pos += 64 + nbytes
    return out, pos


def corrupted(tmp_path):
    """name -> path of a file that must be refused"""
    good = tmp_path / "good.msom"
    write_sample(good)
    b = good.read_bytes()
    recs, trailer = rec_offsets(b)
    assert trailer + 16 == len(b)
    psi_hdr, psi_pay, psi_n = recs[1]
    out = {}

    def put(name, data):
        out[name] = tmp_path / f"{name}.msom"
        out[name].write_bytes(bytes(data))

    put("empty", b"")
    put("cut_in_header", b[:40])
    put("cut_in_params", b[:70])
    put("cut_in_record_header", b[:psi_hdr + 20])
    put("cut_in_payload", b[:psi_pay + psi_n // 2])
    put("cut_before_trailer", b[:trailer])
    put("cut_in_trailer", b[:trailer + 9])
    x = bytearray(b); x[psi_pay + 8 * 37 + 3] ^= 0x10; put("flipped_payload_byte", x)
    x = bytearray(b)   # rows 1 and 2 of layer 0 of psi change places: the same numbers at other positions
    r1, r2 = psi_pay + 16 * 8, psi_pay + 2 * 16 * 8
    x[r1:r1 + 128], x[r2:r2 + 128] = b[r2:r2 + 128], b[r1:r1 + 128]
    put("rows_swapped", x)
    x = bytearray(b); x[0:4] = b"XSOM"; put("bad_magic", x)
    x = bytearray(b); struct.pack_into("<I", x, 8, 2); put("version_plus_1", x)
    x = bytearray(b); struct.pack_into("<Q", x, psi_hdr + 40, 1 << 40); put("byte_count_beyond_file", x)
    x = bytearray(b); struct.pack_into("<I", x, psi_hdr + 20, 3000); struct.pack_into("<Q", x, psi_hdr + 40, 3000 * 8 * 16 * 8); put("shape_beyond_file", x)
    x = bytearray(b); struct.pack_into("<I", x, 48, 4000); put("too_many_records", x)
    x = bytearray(b); x[trailer + 8] ^= 1; put("trailer_sum", x)
    return good, out


def test_corrupted_files_are_refused(tmp_path):
    good, bad = corrupted(tmp_path)
    assert api.state_check(good) == 5
    assert len(bad) >= 12
    for name, p in bad.items():
        with pytest.raises(api.MsomError) as e:
            api.state_check(p)
        assert e.value.code == MSOM_ERR_IO, name
        assert len(str(e.value)) > len("error -2: ") and p.name in str(e.value), (name, str(e.value))
        with pytest.raises(StateFormatError):
            read_state(p)
    # info reads the structure without the payloads: it refuses what breaks the structure, never crashes on the rest
    for name, p in bad.items():
        try:
            api.state_info(p)
        except api.MsomError as e:
            assert e.code == MSOM_ERR_IO, name


def test_sanitizer_build_of_the_reader(tmp_path):
    """state_io.c with its own main (driver/state_check.c) under -fsanitize=address,undefined, a stand-alone program"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler: the sanitizer build of state_io.c did not run")
    exe = tmp_path / "state_check_san"
    cmd = [cc, "-g", "-O1", "-std=gnu99", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(CSRC, "driver", "state_check.c"), os.path.join(CSRC, "state_io.c"), os.path.join(CSRC, "params.c"), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"asan|ubsan|sanitize", r.stderr, re.I):
        pytest.skip("the host compiler has no sanitizer runtime: the sanitizer build of state_io.c did not run")
    assert r.returncode == 0, r.stderr
    good, bad = corrupted(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(good), GOLDEN], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and r.stdout.count(": ok, version 1") == 2 and not r.stderr, r.stdout + r.stderr
    for name, p in bad.items():
        r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 1 and "refused (-2)" in r.stdout and not r.stderr, (name, r.stdout, r.stderr)


# ------------------------------------------------------------------ the golden file

def test_golden_file_is_version_1_and_what_the_oracle_gives():
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert api.state_check(GOLDEN) == 3
    i = api.state_info(GOLDEN)
    assert (i["version"], i["dialect"], i["nx"], i["ny"], i["nl"], i["iter"], i["names"]) == (1, 0, 32, 32, 3, 3, ["time", "psi", "q"])
    d, want = read_state(GOLDEN), golden_content()
    assert d["params"] == want["params"]
    assert (d["t"], d["dt"], d["previous"], d["iter"]) == (want["t"], want["dt"], want["previous"], want["iter"])
    for k in ("psi", "q"):
        assert np.array_equal(d["records"][k], want["records"][k]), k
    # byte for byte: the writer of today makes the file of the day it was committed
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        write_state(os.path.join(t, "g.msom"), **want)
        assert open(os.path.join(t, "g.msom"), "rb").read() == open(GOLDEN, "rb").read()


# ------------------------------------------------------------------ the header and the table of the GPU file

def state_header_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msom_state.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(msom_[a-z0-9_]+)\s*\(", txt)))
    takes = {n for n in names if re.search(r"\b" + n + r"\s*\(\s*msom_t\s*\*", txt)}
    return names, takes


def test_every_state_entry_point_has_a_row():
    from test_gpu_state import STATE_ROWS
    names, takes = state_header_symbols()
    assert set(names) - takes == {"msom_create_from_state", "msom_state_check", "msom_state_info"}
    assert takes == {"msom_state_save", "msom_state_load", "msom_state_dbg_flip"}
    assert set(STATE_ROWS) == takes, sorted(set(STATE_ROWS) ^ takes)
    assert STATE_ROWS["msom_state_save"] == "pure" and STATE_ROWS["msom_state_load"] == "mutating"


@pytest.mark.parametrize("strict", [False, True])
def test_library_exports_the_state_header(strict):
    L = api.load_library(strict=strict)
    for n in state_header_symbols()[0]:
        assert hasattr(L, n), n


def test_msom_h_names_the_new_header_without_declaring_it():
    txt = open(os.path.join(ROOT, "include", "msom.h")).read()
    assert "msom_state.h" in txt
    from test_cabi_host import declared_symbols
    assert not [n for n in declared_symbols() if n.startswith("msom_state") or n == "msom_create_from_state"]


if __name__ == "__main__":
    if sys.argv[1:] == ["--make-golden"]:
        make_golden()
        print("wrote", GOLDEN)
