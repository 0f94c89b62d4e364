#!/usr/bin/env python3
"""Records tests/golden/item_records_parent.npz: the cases of tests/test_gpu_item_records.py run on the
GPU with the library of the commit BEFORE the item records (the walk that gathered its own set-up).

    NDPP_HIP_LIB=/path/to/that/libndpp_hip.so python tools/make_item_records_golden.py [OUT.npz]

The fixture holds, per case, the seed and the length of its inputs and the moments and status words.
Without NDPP_HIP_LIB the tree's own library is used -- which only re-records what the test then
compares with itself, so the script insists on the variable."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    if not os.environ.get("NDPP_HIP_LIB"):
        raise SystemExit("set NDPP_HIP_LIB to the parent commit's libndpp_hip.so")
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "item_records_parent.npz"
    import ndpp_amd
    import test_gpu_item_records as T
    ndpp_amd.load()
    arrays = {}
    for name in sorted(T.CASES):
        out, status = T.run_case(ndpp_amd, name, os.environ.__setitem__, os.environ.pop)
        arrays[f"seed_{name}"] = np.int64(T.CASES[name][0])
        arrays[f"n_{name}"] = np.int64(T.CASES[name][1])
        arrays[f"out_{name}"] = out
        arrays[f"status_{name}"] = status
        print(f"{name}: out {out.shape} finite {bool(np.isfinite(out).all())} status {np.unique(status).tolist()}")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out_path, **arrays)
    print("wrote", out_path, out_path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
