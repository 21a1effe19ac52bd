"""Records tests/golden/cache_refusals.json: what the handle-based entries of ce_cache.hip answer to the calls of
tests/cache_refusal_cases.py, taken from the library of the checkout given by --repo (default: this one).

    python tests/golden/record_cache_refusals.py --part create --repo <checkout with its own build> --commit <its hash>
    python tests/golden/record_cache_refusals.py --part handle --repo <the same checkout> --commit <its hash>

`create` (ce_cache_create's bad configurations) passes made-up addresses: run it where no GPU is visible.  `handle`
(every other entry, on one tiny cache per eviction strategy) needs the GPU.  Either part is merged into the fixture that
is already there.  The fixture holds one number per case: an index into `answers`, the list of the distinct (return
value, message) pairs; the message is null where nothing was refused or the first HIP call itself failed.  The fixture
in the repository was recorded from the parent of the commit that gave the cache op one call record."""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["create", "handle"])
    ap.add_argument("--repo", default=str(HERE.parent.parent))
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=str(HERE / "cache_refusals.json"))
    a = ap.parse_args()
    sys.path.insert(0, a.repo)                        # the package under test
    sys.path.insert(1, str(HERE.parent))              # the case generator
    import torch

    import cache_refusal_cases as cc
    from cachedembedding_amd import _lib
    assert Path(_lib.__file__).resolve().is_relative_to(Path(a.repo).resolve())
    out = Path(a.out)
    fix = json.loads(out.read_text()) if out.exists() else {"answers": []}
    assert fix.setdefault("commit", a.commit) == a.commit, "the fixture holds answers of another commit"
    answers = fix["answers"]

    def index(rows):
        idx = []
        for _, rc, msg in rows:
            if [rc, msg] not in answers:
                answers.append([rc, msg])
            idx.append(answers.index([rc, msg]))
        return idx

    if a.part == "create":
        assert not torch.cuda.is_available(), "made-up addresses: record where no GPU is visible"
        rows = cc.run_create(_lib)
        fix["create"] = {"singles": [label for label, _, _ in cc.CREATE_SINGLES], "rows": index(rows)}
        print("create:", len(rows), "cases")
    else:
        fix["handle"] = {}
        for strategy in cc.STRATEGIES:
            rows = cc.run_handle(_lib, strategy)
            fix["handle"][strategy] = {"labels": [label for label, _, _ in rows], "rows": index(rows)}
            print("handle,", strategy + ":", len(rows), "cases")
    with open(out, "w") as f:
        json.dump(fix, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, out.stat().st_size, "bytes,", len(answers), "distinct answers")


if __name__ == "__main__":
    main()
