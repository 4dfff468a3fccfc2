"""The state file of include/msom_state.h and include/msomn_state.h in pure Python, written from the format text of DESIGN.md ("State file"), not by calling
the library: `read_state` and `write_state` are the independent statement of the format (the tests hold the library to them), and
`write_state` is how a user builds an fp64 initial state for `QG.load_state` or `NodeQG.load_state`.

Dialects: 0 msqg and 1 newqg (cell-centred, nx x ny cells), 2 the vertex model (nx = ny = N + 1 vertices; its noise is a cell scalar,
a field record with its own shape (1, N, N): a record's ny and nx are its own and need not be the header's).

Layout (little-endian):
  header   64 bytes: magic "MSOMSTAT", then 12 uint32: version, dialect, nx, ny, nl, nptr, stochastic, noise_mode, mode_pv_invert,
           flag_topo, nrecords, params_len; 8 zero bytes
  params   params_len bytes of params.in text, zero-padded to a multiple of 8
  record   64-byte header: name[16] NUL-padded, uint32 kind (0 field, 1 scalars), layers, ny, nx, ring, 0; uint64 nbytes, digest, 0;
           then nbytes of fp64, [layer][y][x] (ring = 1: [layer][ny + 2][nx + 2], ghost cells included)
  trailer  "MSOMEND\\0", uint64 sum of the record digests mod 2^64
"""
import struct
from collections import OrderedDict

import numpy as np

MAGIC = b"MSOMSTAT"
ENDTAG = b"MSOMEND\0"
VERSION = 1
KIND_FIELD, KIND_SCALARS = 0, 1
HEADER_KEYS = ("version", "dialect", "nx", "ny", "nl", "nptr", "stochastic", "noise_mode", "mode_pv_invert", "flag_topo")
TIME_KEYS = ("t", "dt", "previous", "tnext", "iter")   # the scalars of record "time", in this order
# dialect 2, a handle with running statistics (msomn_stats_begin): field record k holds accumulator MSOM_ST_k (the selected ones are
# written, [nl][N + 1][N + 1]), and the scalars of record "stats" in this order
NODE_STATS_RECORDS = ("st_psi", "st_q", "st_psi2", "st_q2", "st_ke", "st_uq", "st_vq")
NODE_STATS_KEYS = ("mask", "count", "every", "on", "W", "samples")


class StateFormatError(ValueError):
    pass


def _mix64(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest(a):
    """D = sum_k mix64(bits(x_k) + 0x9E3779B97F4A7C15 (k + 1)) mod 2^64 over the array in C order"""
    bits = np.ascontiguousarray(a, dtype="<f8").reshape(-1).view(np.uint64)
    with np.errstate(over="ignore"):
        k1 = np.arange(1, bits.size + 1, dtype=np.uint64)
        return int(_mix64(bits + np.uint64(0x9E3779B97F4A7C15) * k1).sum(dtype=np.uint64))


def write_state(path, records, nx, ny, nl, params="", dialect=0, nptr=0, stochastic=0, noise_mode=0, mode_pv_invert=0, flag_topo=0,
                t=0.0, dt=1.0, previous=0.0, tnext=float("inf"), iter=0, ring=(), cells=()):
    """Write a state file.  records: name -> array; a 3-d array of shape (layers, ny, nx) is a field record (names in `ring`:
    (layers, ny + 2, nx + 2) with the ghost cells; names in `cells`: (layers, ny - 1, nx - 1), a field on the cells between the
    vertices of a dialect-2 file, stored with its own ny - 1 and nx - 1), a 1-d array a record of scalars.  The record "time" is
    made from t, dt, previous, tnext, iter unless `records` brings its own."""
    recs = OrderedDict()
    if "time" not in records:
        recs["time"] = np.array([t, dt, previous, tnext, iter], dtype=np.float64)
    for name, a in records.items():
        recs[name] = np.ascontiguousarray(a, dtype=np.float64)
    text = params.encode() if isinstance(params, str) else bytes(params)
    out = [MAGIC, struct.pack("<12I", VERSION, dialect, nx, ny, nl, nptr, stochastic, noise_mode, mode_pv_invert, flag_topo, len(recs), len(text)),
           b"\0" * 8, text, b"\0" * (-len(text) % 8)]
    dsum = 0
    for name, a in recs.items():
        nm = name.encode()
        if not 0 < len(nm) <= 16:
            raise StateFormatError(f"record name {name!r}: 1 to 16 bytes")
        g = 2 if name in ring else 0
        ry, rx = (ny - 1, nx - 1) if name in cells else (ny, nx)
        if a.ndim == 1:
            kind, shape = KIND_SCALARS, (a.size, 1, 1)
        elif a.ndim == 3 and a.shape[1:] == (ry + g, rx + g):
            kind, shape = KIND_FIELD, (a.shape[0], ry, rx)
        else:
            raise StateFormatError(f"record {name!r}: shape {a.shape} is neither 1-d nor (layers, {ry + g}, {rx + g})")
        d = digest(a)
        dsum = (dsum + d) % 2**64
        out += [nm.ljust(16, b"\0"), struct.pack("<6I3Q", kind, *shape, 1 if g else 0, 0, a.nbytes, d, 0), a.astype("<f8").tobytes()]
    out += [ENDTAG, struct.pack("<Q", dsum)]
    with open(path, "wb") as f:
        f.write(b"".join(out))


def read_state(path, verify=True):
    """The file as a dict: the header keys, "params" (str), "records" (name -> array, fields as (layers, ny, nx) or with the ring
    (layers, ny + 2, nx + 2), scalars 1-d), "digests", "ring" (names stored with their ring), and t, dt, previous, tnext, iter of
    the record "time" when it is there.  verify: every digest and the trailer are checked (StateFormatError)."""
    with open(path, "rb") as f:
        b = f.read()
    if len(b) < 64:
        raise StateFormatError("short file: no header")
    if b[:8] != MAGIC:
        raise StateFormatError("bad magic")
    h = struct.unpack_from("<12I", b, 8)
    out = dict(zip(HEADER_KEYS, h[:10]))
    if out["version"] != VERSION:
        raise StateFormatError(f"unknown version {out['version']}")
    nrec, plen = h[10], h[11]
    pos = 64
    if pos + plen + (-plen % 8) > len(b):
        raise StateFormatError("short file: params")
    out["params"] = b[pos:pos + plen].decode()
    pos += plen + (-plen % 8)
    recs, digs, rings, dsum = OrderedDict(), OrderedDict(), [], 0
    for _ in range(nrec):
        if pos + 64 > len(b):
            raise StateFormatError("short file: record header")
        name = b[pos:pos + 16].rstrip(b"\0").decode()
        kind, layers, ny, nx, ring, _r0, nbytes, d, _r1 = struct.unpack_from("<6I3Q", b, pos + 16)
        pos += 64
        g = 2 if ring else 0
        if nbytes != 8 * layers * (ny + g) * (nx + g) or pos + nbytes > len(b):
            raise StateFormatError(f"record {name!r}: {nbytes} bytes do not fit its shape or the file")
        a = np.frombuffer(b, dtype="<f8", count=nbytes // 8, offset=pos).astype(np.float64)
        pos += nbytes
        if verify and digest(a) != d:
            raise StateFormatError(f"record {name!r}: digest mismatch")
        recs[name] = a if kind == KIND_SCALARS else a.reshape(layers, ny + g, nx + g)
        digs[name] = d
        if ring:
            rings.append(name)
        dsum = (dsum + d) % 2**64
    if pos + 16 > len(b) or b[pos:pos + 8] != ENDTAG:
        raise StateFormatError("short file: no trailer")
    if verify and struct.unpack_from("<Q", b, pos + 8)[0] != dsum:
        raise StateFormatError("trailer does not hold the sum of the record digests")
    out.update(records=recs, digests=digs, ring=rings)
    if "time" in recs and recs["time"].size >= 5:
        out.update(zip(TIME_KEYS, (float(v) for v in recs["time"][:5])))
        out["iter"] = int(out["iter"])
    return out
