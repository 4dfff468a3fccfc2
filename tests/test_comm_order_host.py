"""The order in which a halo exchange posts its messages and the rule that pairs them (msom_amd/csrc/comm_order_inl.h: comm_post_order,
comm_pair -- RCCL's rule, which the in-process transport of the tiled tests applies too) against brute force over every rank and message
of 50 tile grids, in a stand-alone program built with AddressSanitizer and UBSan (tools/comm_order_host_check.cpp).  No GPU.

Neighbour ranks follow create_common, where a single tile has no neighbours at all, periodic or not: the two 1 x 1 topologies of the
enumerated set post empty lists.  A tile that is its own peer on every face exists only in msom_dbg_rccl_selftest; its list is checked
beside the set (with the project's rule, and that both wrong rules fail on it), not in it, because 'receives by descending tag' is
wrong on that list although it holds faces only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_posting_order_pairs_every_halo_with_the_opposite_edge_under_sanitizers(tmp_path):
    exe = str(tmp_path / "comm_order_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "comm_order_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-12000:], r.stderr[-4000:])
    assert r.returncode == 0
    out = r.stdout
    # px, py in {1, 2, 3, 4, 8}, walled and periodic: 50 topologies x the lists {W,E}, {S,N}, {W,E,S,N}, all eight directions
    topo = re.findall(r"^(walled|periodic) (\d)x(\d): (\d+) messages: ok$", out, re.M)
    assert len(topo) == 50 and len(set(topo)) == 50
    assert {(w, int(a), int(b)) for w, a, b, _ in topo} == {(w, a, b) for w in ("walled", "periodic") for a in (1, 2, 3, 4, 8) for b in (1, 2, 3, 4, 8)}
    assert "FAIL" not in out and "NOT refused" not in out
    total = sum(int(n) for *_, n in topo)
    assert f"50 topologies, 200 lists, {total} messages checked, 0 failures" in out and total > 0
    # the single tile is in the set (no messages, as create_common wires it), and as its own peer beside it
    assert "walled 1x1: 0 messages: ok" in out and "periodic 1x1: 0 messages: ok" in out
    assert "one rank its own peer in every direction: 16 messages: ok" in out
    # a full periodic grid of P tiles posts 2 + 2 + 4 + 8 messages per tile
    for w, a, b, n in topo:
        if w == "periodic" and int(a) * int(b) > 1:
            assert int(n) == 16 * int(a) * int(b), (w, a, b, n)
    # wrong rule 1, receives in the order of the sends: a halo for the wrong edge wherever one peer gets both messages of an axis
    for t in ("2x1", "1x2", "2x2"):
        for s in ("WE", "SN"):
            assert f"same-order caught: periodic {t} {s} (tag)" in out
    assert not re.search(r"same-order caught: walled", out)   # between walls no peer ever gets two messages of one list
    # wrong rule 2, receives by descending tag: right on every list of faces, caught only by the eight directions
    assert "descending caught: periodic 2x1 all8" in out
    desc = re.findall(r"descending caught: (.*)$", out, re.M)
    assert desc and all(d.endswith(" all8") for d in desc)
    assert re.search(r"caught on %d lists, 0 of them face-only" % len(desc), out)
    # broken lists
    assert "broken list 'one message dropped': refused with the number error" in out
    assert "broken list 'one count changed': refused with the count error" in out
    # the function posts what the loops it replaced posted
    assert out.count("| before the move:") == 4
    for line in re.findall(r"^periodic 2x2 WESN rank \d: (.*)$", out, re.M):
        new, old = line.split(" | before the move: ")
        assert new == old == "so 0 1 2 3 ro 1 0 3 2"
