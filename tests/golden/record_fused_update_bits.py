"""Records tests/golden/fused_update_bits.npz: the bits of the fused optimizer updates (ce_bag_adagrad.hip) for the
cases of tests/fused_update_cases.py, taken from the library of the checkout given by --repo (default: this one).

    python tests/golden/record_fused_update_bits.py --repo <checkout with its own build> --commit <its hash> [--out F]

It drives the public Python API only, so it runs against any commit that has accumulator=.  Before
anything is written it asserts that both paths of a case (accumulator="cache" and "step") gave the same bits on that
library: the fixture holds one set of bits per case and both paths are held to it.
The fixture in the repository was recorded from the parent of the commit that made the atomic paths' row update one
function (with two further cases of the sorted path, cut off since: its arrays are the first 45 cases of that
recording)."""
import argparse
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=str(HERE.parent.parent))
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=str(HERE / "fused_update_bits.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.repo)                        # the package under test
    sys.path.insert(1, str(HERE.parent))              # the case generator
    import cachedembedding_amd
    import fused_update_cases as fc
    assert Path(cachedembedding_amd.__file__).resolve().is_relative_to(Path(a.repo).resolve())
    names, crcs, moms = [], [], []
    for i, case in enumerate(fc.cases()):
        got = {p: fc.run(case, i, p) for p in case.paths}
        crc, mom = got[case.paths[0]]
        for p in case.paths[1:]:
            assert not fc.differing_rows(got[p][0], crc), (case.name, p, "weight", fc.differing_rows(got[p][0], crc))
            if mom is not None:
                assert np.array_equal(got[p][1], mom), (case.name, p, "momentum")
        assert (crc[0] != crc[1]).any() and (crc[1] != crc[2]).any(), case.name
        names.append(case.name)
        crcs.append(crc)
        moms.append(mom if mom is not None else np.zeros_like(crc))
        print(case.name, "/".join(case.paths), "ok", flush=True)
    from cachedembedding_amd.build import _hipcc
    hipcc = subprocess.run([_hipcc(), "--version"], capture_output=True, text=True).stdout.strip()
    np.savez_compressed(a.out, names=np.array(names), crc=np.stack(crcs), momentum=np.stack(moms),
                        commit=np.array(a.commit), hipcc=np.array(hipcc))
    print("wrote", a.out, Path(a.out).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
