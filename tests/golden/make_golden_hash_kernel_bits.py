"""Record tests/golden/hash_kernel_bits.json: one SHA-256 per input and output buffer of every case of
tests/test_gpu_hash_kernel_bits.py, with the commit and the identity of the library they were taken from.

Run it on the MI355X with the library of the commit BEFORE a change that must not move a bit, never with the code under test, twice,
and keep the file only when both runs wrote the same hashes:

    python tests/golden/make_golden_hash_kernel_bits.py --commit <sha of that commit> [--lib path [--stamp path]] [--out path]

(the commit is an argument because the tree this runs in need not be a git checkout; --lib names that commit's library when the
tree's own dynhor_amd/libdynhor_hip.so is already built from the changed sources, --stamp its libdynhor_hip.build.json).  Every case
is also run twice in the process and must agree with itself.  A differing hash in the test is a finding to explain; it is never a
reason to run this again.
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
    ap.add_argument("--out", default=os.path.join(HERE, "hash_kernel_bits.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    from dynhor_amd import _lib
    if args.lib:                                                # before the first _lib.lib(): every call then goes to this library
        assert _lib._LIB is None
        _lib.LIB_PATH = entry.LIB = os.path.abspath(args.lib)
        entry.STAMP = os.path.abspath(args.stamp) if args.stamp else os.devnull
    from tests import test_gpu_hash_kernel_bits as B
    lib_sha, stamp = entry.lib_identity()
    out = {"commit": args.commit, "lib_sha16": lib_sha, "sources_sha16": (stamp or {}).get("sources_sha16"),
           "hipcc": (stamp or {}).get("hipcc"), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hashes": {}}
    for case in B.CASES:
        first, second = B.hashes(case), B.hashes(case)
        assert first == second, f"{case}: two runs differ: {[k for k in first if first[k] != second[k]]}"
        assert first["weight_grads_finite"], f"{case}: the table gradient is not finite"
        out["hashes"][case] = first
        print(case, {k: (v[:12] if isinstance(v, str) else v) for k, v in first.items()}, flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
