"""A PERCENTILE column of a data table is an OBJECT holding a DoubleArrayList: object type 3, a big-endian int size, then big-endian doubles
(ObjectSerDeUtils.java:482-511).  tests/datatable_percentile_main.cpp hands a hand-built list of (value, count) runs — with -0.0, 0.0 and
NaN — to the library's host-side writer (pg_datatable.cpp, no device); the bytes are decoded here by the test's own few lines."""
import os
import struct
import subprocess

import pytest

from oracle import po_datatable as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = [float("-inf"), -0.0, 0.0, 1.5, float("nan")]
COUNTS = [2, 1, 3, 1, 2]


def test_double_array_list_bytes_of_a_hand_built_list(tmp_path, monkeypatch):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "datatable_percentile")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-x", "hip", "-I" + csrc,
                           os.path.join(ROOT, "tests", "datatable_percentile_main.cpp"), os.path.join(csrc, "pg_datatable.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    table = bytes.fromhex(out.stdout.strip())
    seen = []
    inner = dt.deserialize_object

    def decode(kind, b):   # the test's own decoder of object type 3
        if kind != 3:
            return inner(kind, b)
        seen.append(bytes(b))
        n = struct.unpack_from(">i", b, 0)[0]
        assert len(b) == 4 + 8 * n
        return list(struct.unpack_from(f">{n}d", b, 4))
    monkeypatch.setattr(dt, "deserialize_object", decode)
    t = dt.parse_data_table_v4(table)
    assert t["names"] == ["count(*)", "percentile(lat, 99.9)"] and t["types"] == ["LONG", "OBJECT"]
    assert len(t["rows"]) == 1 and t["rows"][0][0] == 9
    # the runs expanded, ascending, every double bit for bit: -0.0 keeps its sign, NaN is the canonical quiet NaN
    expanded = [v for v, c in zip(VALUES, COUNTS) for _ in range(c)]
    want = struct.pack(">i", len(expanded)) + b"".join(struct.pack(">d", v) for v in expanded)
    assert seen == [want]
    assert want[4 + 8 * 2:4 + 8 * 3] == bytes.fromhex("8000000000000000") and want[-8:] == bytes.fromhex("7ff8000000000000")
    # ... and the object's type int in front of it is 3
    assert struct.pack(">i", 3) + want in table
