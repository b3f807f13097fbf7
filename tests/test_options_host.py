"""dicp_set_option / dicp_get_option on the built library (host only, no device work): every
option of include/difficp_hip.h with its default, its range or set, and what is refused."""
import ctypes as C
import os
import re
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difficp_hip.h")
LIB = os.path.join(ROOT, "diff-icp_amd", "libdifficp_hip.so")
OK, INVALID = 0, 1
INT_MAX = 2**31 - 1

# name: (default, allowed values' range (lo, hi) or the allowed set), in the header's order.
# min_chunk: 0 (automatic) or 16 .. 65536
OPTIONS = {
    "fwd_alg": (2, (0, 6)),
    "bwd_alg": (3, (0, 3)),
    "bwd_eta_alg": (2, (0, 2)),
    "r_fwd": (2, {1, 2, 4}),
    "r_bwd": (1, {1, 2, 4}),
    "split_rounds": (0, (0, 64)),
    "force_splits": (0, (0, 65536)),
    "sym_L": (0, (0, 64)),
    "min_chunk": (0, (16, 65536)),
    "pk_rp": (0, (0, 2)),
    "sym_rp": (0, (0, 2)),
    "red_alg": (1, (0, 2)),
    "sym_red": (1, (0, 2)),
    "sym_red_rows": (0, {0, 4, 8}),
    "sym_fwd_rows": (0, {0, 4, 6, 8}),
    "pair_cutoff": (1, (0, 2)),
    "pair_cutoff_log2": (48, (8, 150)),
    "lse_pk": (1, (0, 1)),
    "lse_adapt": (1, (0, INT_MAX)),
    "lse_bound": (1, (0, 1)),
    "cx_rho_x100": (150, (0, 100000)),
    "mfma_rmax_x100": (300, (0, INT_MAX)),
    "ext_alg": (1, (0, 1)),
    "batch_share": (1, (1, 4096)),
    "coord_raw": (0, (0, 1)),
}
PER_THREAD = ("batch_share", "coord_raw")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built (run __graft_entry__.build())")
    h = C.CDLL(LIB)
    h.dicp_set_option.argtypes = [C.c_char_p, C.c_int]
    h.dicp_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    h.dicp_last_error.restype = C.c_char_p
    return h


def get(lib, name):
    v = C.c_int(-12345)
    assert lib.dicp_get_option(name.encode(), C.byref(v)) == OK, name
    return v.value


def accepted_and_refused(name):
    """(values that must round-trip, values that must be refused) of an option."""
    allowed = OPTIONS[name][1]
    if isinstance(allowed, set):
        lo, hi = min(allowed), max(allowed)
        return sorted(allowed), [v for v in range(lo - 1, hi + 2) if v not in allowed]
    lo, hi = allowed
    good, bad = [lo, hi], [lo - 1] + ([hi + 1] if hi < INT_MAX else [])
    if name == "min_chunk":
        good, bad = [0] + good, [-1, 1] + bad
    return good, bad


def test_header_lists_the_options_in_order():
    """The knob list of the header names exactly the library's options, in the table's order,
    each with its default."""
    text = open(HEADER).read()
    doc = text[text.index("/* Tuning / A-B knobs"):text.index("int dicp_set_option")]
    listed = re.findall(r'^ \*   "(\w+)"\s+\(default (\d+)', doc, flags=re.M)
    assert [n for n, _ in listed] == list(OPTIONS)
    assert {n: int(d) for n, d in listed} == {n: d for n, (d, _) in OPTIONS.items()}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_option_default_range_and_refusals(lib, name):
    default = OPTIONS[name][0]
    assert get(lib, name) == default
    good, bad = accepted_and_refused(name)
    try:
        for v in good:
            assert lib.dicp_set_option(name.encode(), v) == OK, (name, v)
            assert get(lib, name) == v
        for v in bad:
            assert lib.dicp_set_option(name.encode(), v) == INVALID, (name, v)
            assert get(lib, name) == good[-1], (name, v)   # the stored value is unchanged
    finally:
        assert lib.dicp_set_option(name.encode(), default) == OK
    assert get(lib, name) == default


def test_unknown_name_and_null_are_refused_with_a_message(lib):
    v = C.c_int(7)
    for value in (0, 1, 3):   # whatever the value
        lib.dicp_get_option(None, None)   # another message in between
        assert lib.dicp_set_option(b"no_such_option", value) == INVALID
        assert b"no_such_option" in lib.dicp_last_error()
    lib.dicp_set_option(b"no_such_option", 1)
    assert lib.dicp_get_option(b"no_such_name", C.byref(v)) == INVALID
    assert b"no_such_name" in lib.dicp_last_error() and v.value == 7
    assert lib.dicp_get_option(None, C.byref(v)) == INVALID
    assert b"NULL" in lib.dicp_last_error()
    assert lib.dicp_get_option(b"fwd_alg", None) == INVALID
    assert lib.dicp_set_option(None, 1) == INVALID


@pytest.mark.parametrize("name", PER_THREAD)
def test_per_thread_options(lib, name):
    """A per-thread option set on one host thread is not seen by another: a new thread starts
    from the default, and what it sets does not reach the thread that started it."""
    default, (lo, hi) = OPTIONS[name]
    other = hi if default != hi else lo
    seen = []

    def worker():
        seen.append(get(lib, name))
        seen.append(lib.dicp_set_option(name.encode(), other))
        seen.append(get(lib, name))

    def run():
        del seen[:]
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        return list(seen)

    try:
        assert run() == [default, OK, other] and get(lib, name) == default
        assert lib.dicp_set_option(name.encode(), other) == OK
        assert run() == [default, OK, other] and get(lib, name) == other
    finally:
        assert lib.dicp_set_option(name.encode(), default) == OK
