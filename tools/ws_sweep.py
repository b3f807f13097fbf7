#!/usr/bin/env python3
"""Every LDDMM workspace size and split count the library reports, one JSON line per case.

Host-only: calls dicp_workspace_bytes and dicp_num_splits, launches no kernel.  The output of
two builds of the library on the same machine must be byte-identical when a change is meant
to leave the kernel dispatch alone (with a GPU the occupancies are the real ones; without, the
library's fallbacks):

    tools/ws_sweep.py [--lib PATH/libdifficp_hip.so] > sweep.jsonl
"""
import argparse
import ctypes as C
import json
import os

SIZES = (1, 255, 257, 700, 2049, 20000, 33001, 100000)
COUNTS = (1, 2, 3, 8)   # slices of the rows / phased kinds, parts of the part kind
# (kind, name) as in difficp_hip.h
RED, SELF_FWD, SELF_BWD, EXT_FWD, EXT_BWD, FWD_ROWS, BWD_PART, FWD_PHASED = 0, 1, 2, 3, 4, 9, 10, 12
OPTIONS = (("fwd_alg", range(7)), ("bwd_alg", range(4)), ("bwd_eta_alg", range(3)), ("r_fwd", (1, 2, 4)),
           ("r_bwd", (1, 2, 4)), ("ext_alg", (0, 1)), ("pk_rp", range(3)))


def cases():
    """(kind, M, N) of dicp_workspace_bytes."""
    for m in SIZES:
        yield SELF_FWD, m, m
        yield SELF_BWD, m, m
        for n in SIZES:
            for kind in (RED, EXT_FWD, EXT_BWD):
                yield kind, m, n
        for c in COUNTS:
            rows = -(-m // c)
            yield FWD_ROWS, rows, m
            yield FWD_PHASED, rows, m
            yield BWD_PART, m, c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--lib", default=os.path.join(here, "..", "diff-icp_amd", "libdifficp_hip.so"))
    lib = C.CDLL(ap.parse_args().lib)
    lib.dicp_workspace_bytes.restype = C.c_size_t
    lib.dicp_workspace_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int]
    lib.dicp_num_splits.argtypes = [C.c_int, C.c_int64, C.c_int64]
    lib.dicp_set_option.argtypes = [C.c_char_p, C.c_int]
    lib.dicp_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int)]

    def get(name):
        v = C.c_int()
        assert lib.dicp_get_option(name.encode(), C.byref(v)) == 0, name
        return v.value

    def sweep(opts):
        for kind, m, n in cases():
            for d in (2, 3):
                print(json.dumps({"opts": opts, "kind": kind, "M": m, "N": n, "D": d,
                                  "bytes": lib.dicp_workspace_bytes(kind, m, n, d)}))
        for kind in (RED, SELF_FWD, SELF_BWD):
            for m in SIZES:
                for n in SIZES if kind == RED else (m,):
                    print(json.dumps({"opts": opts, "kind": kind, "M": m, "N": n,
                                      "splits": lib.dicp_num_splits(kind, m, n)}))

    for fs in (0, 3):
        fs0 = get("force_splits")
        assert lib.dicp_set_option(b"force_splits", fs) == 0
        sweep({"force_splits": fs})
        for name, values in OPTIONS:
            before = get(name)
            for v in values:
                assert lib.dicp_set_option(name.encode(), v) == 0, (name, v)
                sweep({"force_splits": fs, name: v})
            assert lib.dicp_set_option(name.encode(), before) == 0
        assert lib.dicp_set_option(b"force_splits", fs0) == 0


if __name__ == "__main__":
    main()
