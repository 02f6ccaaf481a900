"""Record tests/golden/mesh_kernel_bits.json (or, with --cases and --out, tests/golden/mesh_draw_bits.json): one SHA-256 per input and
output tensor of every case of tests/test_gpu_mesh_kernel_bits.py, with the commit and the identity of the library they were taken from.

Run it on the MI355X with the library of the commit BEFORE a change that must not move a bit, never with the code under test:

    python tests/golden/make_golden_mesh_kernel_bits.py --commit <sha of that commit> [--lib path [--stamp path]] [--cases a,b,..] [--out path]

(the commit is an argument because the tree this runs in need not be a git checkout; --lib names that commit's library when the
tree's own dynhor_amd/libdynhor_hip.so is already built from the changed sources, --stamp its libdynhor_hip.build.json; --cases
records only the named cases; by default those the test reads from --out, so new cases go into a file of their own and the earlier
recordings stay as they are).  A differing
hash in the test is a finding to explain; it is never a reason to run this again.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the built library belongs to")
    ap.add_argument("--lib", default=None, help="the library to record from (default: the tree's own)")
    ap.add_argument("--stamp", default=None, help="the build stamp that belongs to --lib")
    ap.add_argument("--cases", default=None, help="comma-separated case names (default: the cases the test reads from --out)")
    ap.add_argument("--out", default=os.path.join(HERE, "mesh_kernel_bits.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    from dynhor_amd import _lib
    if args.lib:                                                # before the first _lib.lib(): every wrapper then calls this library
        assert _lib._LIB is None
        _lib.LIB_PATH = entry.LIB = os.path.abspath(args.lib)
        entry.STAMP = os.path.abspath(args.stamp) if args.stamp else os.devnull
    from tests import test_gpu_mesh_kernel_bits as B
    lib_sha, stamp = entry.lib_identity()
    out = {"commit": args.commit, "lib_sha16": lib_sha, "sources_sha16": (stamp or {}).get("sources_sha16"),
           "hipcc": (stamp or {}).get("hipcc"), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hashes": {}}
    # default: the cases the test looks up in the file being written (all of them for a file the test does not know)
    mine = [c for c in B.CASES if os.path.abspath(B.golden_path(c)) == os.path.abspath(args.out)]
    cases = args.cases.split(",") if args.cases else (mine or list(B.CASES))
    unknown = [c for c in cases if c not in B.CASES]
    assert not unknown, f"unknown cases {unknown}; known: {list(B.CASES)}"
    for case in cases:
        first, second = B.hashes(case), B.hashes(case)
        assert first == second, f"{case}: two runs differ: {[k for k in first if first[k] != second[k]]}"
        out["hashes"][case] = first
        print(case, {k: v[:12] for k, v in first.items()}, flush=True)
    if "skip_rules" in cases:
        B.test_skip_rules_reject_four_faces_and_draw_five()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
