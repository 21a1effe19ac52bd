"""Records tests/golden/bag_refusals.json: what every C entry of ce_bag.hip answers to the calls of
tests/bag_refusal_cases.py, taken from the library of the checkout given by --repo (default: this one).

    python tests/golden/record_bag_refusals.py --repo <checkout with its own build> --commit <its hash> [--out F]

Run it where no GPU is visible: the calls pass made-up addresses.  The fixture holds, per entry, the labels of the
single perturbations (the pairs follow from them) and one number per case: an index into `answers`, the list of the
distinct (return value, message) pairs.  The message is null where nothing was refused or the launch itself failed.
The fixture in the repository was recorded from the parent of the commit that gave the bag kernels one launcher
each."""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=str(HERE.parent.parent))
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=str(HERE / "bag_refusals.json"))
    a = ap.parse_args()
    sys.path.insert(0, a.repo)                        # the package under test
    sys.path.insert(1, str(HERE.parent))              # the case generator
    import torch

    import bag_refusal_cases as bc
    from cachedembedding_amd import _lib
    assert Path(_lib.__file__).resolve().is_relative_to(Path(a.repo).resolve())
    assert not torch.cuda.is_available(), "made-up addresses: record where no GPU is visible"
    answers, entries = [], {}
    for entry in bc.ENTRIES:
        rows = []
        for _, rc, msg in bc.run(_lib.lib, _lib.last_error, entry):
            if [rc, msg] not in answers:
                answers.append([rc, msg])
            rows.append(answers.index([rc, msg]))
        entries[entry] = {"singles": [label for label, _, _ in bc.singles(entry)], "rows": rows}
        print(entry, len(rows), "cases", flush=True)
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "answers": answers, "entries": entries}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", a.out, Path(a.out).stat().st_size, "bytes,", len(answers), "distinct answers")


if __name__ == "__main__":
    main()
