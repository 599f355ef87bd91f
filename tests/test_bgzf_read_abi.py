"""CPU-only: the BGZF read entries of the product library that need no GPU -- the index from a member table, its info, members and
virtual offsets, equal to the host build's --, and every argument error of the read and build entries, decided before a context or
a device is touched."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import bgzf_read_cases as brc  # noqa: E402
import bgzfread_binding as hb  # noqa: E402
import deflate_amd as da  # noqa: E402
from test_bgzf_read_cases import FROM_MEMBERS  # noqa: E402


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(da.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deflate-rs_amd"), "-s"])
    return da.load()


def rows_of(tab):
    return [dict(in_off=o, in_len=n, out_off=p, out_len=z, flags=da.MEMBER_HINTED, status=0) for o, n, p, z in tab]


def test_structs(L):
    assert C.sizeof(da.BgzfInfo) == 40 and C.sizeof(da.SeekRange) == 40 and C.sizeof(da.MemberInfo) == 40


@pytest.mark.parametrize("name,rows,file_len,ok", FROM_MEMBERS, ids=[r[0] for r in FROM_MEMBERS])
def test_from_members_rules(L, name, rows, file_len, ok):
    arr = hb.member_rows(rows)
    h = C.c_void_p(1)
    rc = L.mi355_bgzf_index_from_members(C.cast(arr, C.POINTER(da.MemberInfo)) if rows else None, len(rows), file_len, C.byref(h))
    assert rc == (da.OK if ok else da.E_ARG) and bool(h.value) == ok
    L.mi355_bgzf_index_free(h)
    if not ok:
        with pytest.raises(da.DeflateError) as e:
            da.bgzf_index_from_members([dict(zip(("in_off", "in_len", "out_off", "out_len"), r)) if not isinstance(r, dict) else r for r in rows],
                                       file_len)
        assert e.value.code == da.E_ARG


def test_index_equals_the_host_build(L):
    for file in (brc.small_file(), brc.big_file(), brc.model_file()):
        tab = brc.claims(file)
        ix = da.bgzf_index_from_members(rows_of(tab), len(file))
        host = hb.Index(members=tab, file_len=len(file))
        info = ix.info()
        assert info.pop("host_bytes") >= 40 * len(tab)
        assert info == host.info()
        assert [(m["in_off"], m["in_len"], m["out_off"], m["out_len"], m["status"]) for m in ix.members()] == [t + ("OK",) for t in tab]
        total = info["total"]
        for u in sorted({0, 1, total - 1, total} | {p for _o, _n, p, _z in tab} | {p + z - 1 for _o, _n, p, z in tab if z}):
            rc, v = host.voffset(u)
            assert rc == hb.OK and ix.voffset(u) == v and ix.uoffset(v) == host.uoffset(v)[1]
            if u < total:
                assert ix.uoffset(v) == u
        for v in [(o << 16) | z for o, _n, _p, z in tab] + [(len(file) << 16) | 1, ((tab[3][0] + 1) << 16), total + 1]:
            rc, _u = host.uoffset(v)
            if rc == hb.OK:
                assert ix.uoffset(v) == host.uoffset(v)[1]
            else:
                with pytest.raises(da.DeflateError) as e:
                    ix.uoffset(v)
                assert e.value.code == rc == da.E_ARG
        with pytest.raises(da.DeflateError) as e:
            ix.voffset(total + 1)
        assert e.value.code == da.E_ARG
        # the table through a cap that is too small
        n = C.c_size_t(0)
        arr = (da.MemberInfo * 2)()
        assert L.mi355_bgzf_index_members(ix._h, arr, 2, C.byref(n)) == da.E_OUT_TOO_SMALL and n.value == len(tab)
        ix.close()
    big = da.bgzf_index_from_members([dict(in_off=0, in_len=100, out_off=0, out_len=65537)], 100)
    with pytest.raises(da.DeflateError) as e:
        big.voffset(3)
    assert e.value.code == da.E_UNSUPPORTED


def test_argument_errors_touch_no_device(L):
    """every one of these returns before a context is looked at: a NULL context would otherwise make the default one"""
    file = brc.small_file()
    ix = da.bgzf_index_from_members(rows_of(brc.claims(file)), len(file))
    h, rep, got = C.c_void_p(), da.InflateReport(), C.c_uint64(0)
    buf = C.create_string_buffer(64)
    out = C.cast(buf, C.c_void_p)
    fp = C.cast(C.c_char_p(file), C.c_void_p)
    E = da.E_ARG
    # the builds
    assert L.mi355_bgzf_index_build(None, file, len(file), None, C.byref(rep)) == E
    assert L.mi355_bgzf_index_build(None, file, len(file), C.byref(h), None) == E
    assert L.mi355_bgzf_index_build(None, None, 10, C.byref(h), C.byref(rep)) == E
    assert L.mi355_bgzf_index_build_device(None, fp, len(file), None, C.byref(rep), None) == E
    assert L.mi355_bgzf_index_build_device(None, fp, len(file), C.byref(h), None, None) == E
    assert L.mi355_bgzf_index_build_device(None, None, 10, C.byref(h), C.byref(rep), None) == E
    assert not h.value
    assert L.mi355_bgzf_index_from_members(None, 0, 0, None) == E
    # info, members, offsets
    assert L.mi355_bgzf_index_info(None, C.byref(da.BgzfInfo())) == E and L.mi355_bgzf_index_info(ix._h, None) == E
    assert L.mi355_bgzf_index_members(None, None, 0, C.byref(C.c_size_t())) == E and L.mi355_bgzf_index_members(ix._h, None, 0, None) == E
    assert L.mi355_bgzf_index_members(ix._h, None, 5, C.byref(C.c_size_t())) == E
    assert L.mi355_bgzf_voffset(None, 0, C.byref(got)) == E and L.mi355_bgzf_voffset(ix._h, 0, None) == E
    assert L.mi355_bgzf_uoffset(None, 0, C.byref(got)) == E and L.mi355_bgzf_uoffset(ix._h, 0, None) == E
    L.mi355_bgzf_index_free(None)
    # the reads
    assert L.mi355_bgzf_read_device(None, None, fp, 0, 10, out, C.byref(got), C.byref(rep), None) == E
    assert L.mi355_bgzf_read_device(None, ix._h, None, 0, 10, out, C.byref(got), C.byref(rep), None) == E
    assert L.mi355_bgzf_read_device(None, ix._h, fp, 0, 10, None, C.byref(got), C.byref(rep), None) == E
    assert L.mi355_bgzf_read_device(None, ix._h, fp, 0, 10, out, None, C.byref(rep), None) == E
    assert L.mi355_bgzf_read_device(None, ix._h, fp, 0, 10, out, C.byref(got), None, None) == E
    assert L.mi355_bgzf_read(None, None, file, 0, 10, out, C.byref(got), C.byref(rep)) == E
    assert L.mi355_bgzf_read(None, ix._h, None, 0, 10, out, C.byref(got), C.byref(rep)) == E
    assert L.mi355_bgzf_read(None, ix._h, file, 0, 10, None, C.byref(got), C.byref(rep)) == E
    assert L.mi355_bgzf_read(None, ix._h, file, 0, 10, out, None, C.byref(rep)) == E
    assert L.mi355_bgzf_read(None, ix._h, file, 0, 10, out, C.byref(got), None) == E
    r = (da.SeekRange * 2)()
    r[0].off, r[0].len, r[0].out = 0, 10, out.value
    r[1].off, r[1].len, r[1].out = 5, 10, None
    assert L.mi355_bgzf_read_batch_device(None, ix._h, fp, r, 2, None, None) == E  # a NULL out with len > 0
    assert L.mi355_bgzf_read_batch_device(None, None, fp, r, 1, None, None) == E
    assert L.mi355_bgzf_read_batch_device(None, ix._h, None, r, 1, None, None) == E
    assert L.mi355_bgzf_read_batch_device(None, ix._h, fp, None, 1, None, None) == E
    assert L.mi355_bgzf_read_batch_device(None, ix._h, fp, r, 1 << 31, None, None) == E
    assert (r[0].got, r[0].status) == (0, 0) and buf.raw == bytes(64)
    assert L.mi355_bgzf_last_read(None, (C.c_uint64 * 6)()) == E and L.mi355_bgzf_last_read_stages(None, (C.c_float * 3)()) == E
    # a read through an index of a table needs a context and a file
    with pytest.raises(ValueError):
        ix.read(0, 10)
