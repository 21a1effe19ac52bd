"""Records tests/golden/update_dispatch.json: for every case of tests/update_dispatch_cases.py the C entry that
`_BagFn.backward` of the checkout given by --repo calls, its arguments as data and the workspaces the call allocated.

    python tests/golden/record_update_dispatch.py --repo <checkout with its own build> --commit <its hash> [--out F]
                                                  [--only OPTIMIZER[,OPTIMIZER]]

It needs no GPU (update_dispatch_cases.py says how).  The case builder asks `functional.check_front` what is refused
before the forward, so --repo must be a checkout that has it: none older than the commit that gave the refusals one
rule set.  The cases: the full product of base_cases(), less what embedding_bag refuses before its forward,
then the smaller sweep (variants()) over the first case that reached each entry.  --only records the cases of the named
optimizers again (a new optimizer's, say) and keeps every other record of the file as it is; the file names the commit
each optimizer's records come from.
The fixture in the repository was recorded from the parent of the commit that made the backward plan its call in one
function: regenerating it from the code it checks would prove nothing."""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent

# every entry the backward reaches outside its sparse=True arms and the per_sample_weights gradient: a case set that
# loses one of them must fail here
ENTRIES = """
ce_bag_backward_dense_act ce_bag_backward_dense_src_act
ce_bag_backward_sgd_act ce_bag_backward_sgd_src_act ce_bag_backward_sgd_lrdev ce_bag_backward_sgd_src_lrdev
ce_bag_backward_sgd_sorted
ce_bag_backward_rowwise_adagrad_act ce_bag_backward_rowwise_adagrad_src_act
ce_bag_backward_update_w16 ce_bag_backward_update_src_w16 ce_bag_backward_update_sorted
ce_bag_backward_update_compact ce_bag_backward_update_compact_src
ce_bag_backward_update_lrdev ce_bag_backward_update_src_lrdev
ce_bag_backward_update_wd ce_bag_backward_update_src_wd ce_bag_backward_update_sorted_wd
ce_bag_backward_update_clip ce_bag_backward_update_src_clip ce_bag_backward_update_sorted_clip
ce_bag_backward_adam ce_bag_backward_adam_src ce_bag_backward_adam_wd ce_bag_backward_adam_src_wd
ce_bag_backward_adam_clip ce_bag_backward_adam_src_clip ce_bag_backward_adam_sorted
ce_bag_backward_pradam ce_bag_backward_pradam_src ce_bag_backward_pradam_clip ce_bag_backward_pradam_src_clip
ce_bag_backward_pradam_sorted
ce_bag_backward_adagrad ce_bag_backward_adagrad_src ce_bag_backward_adagrad_sorted
""".split()
MAX_BYTES = 150 * 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=str(HERE.parent.parent))
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=str(HERE / "update_dispatch.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    assert len(ENTRIES) == len(set(ENTRIES)) == 37
    sys.path.insert(0, a.repo)                        # the package under test
    sys.path.insert(1, str(HERE.parent))              # the case generator
    import cachedembedding_amd
    from cachedembedding_amd import functional as F
    import update_dispatch_cases as dc
    assert Path(cachedembedding_amd.__file__).resolve().is_relative_to(Path(a.repo).resolve())
    only = set(filter(None, a.only.split(",")))
    records, commits = [], {}
    if only:
        old = json.loads(Path(a.out).read_text())
        records = [r for r in dc.unpack(old["entries"]) if r[0].optimizer not in only]
        commits = old["recorded_from"]
    refused = 0
    with dc.patched(F) as rec:
        def record(cases):
            nonlocal refused
            new = []
            for case in cases:
                got = dc.run(case, F, rec)
                if got is None:
                    refused += 1
                else:
                    new.append((case,) + got)
            return new
        base = record(c for c in dc.base_cases() if not only or c.optimizer in only)
        first = {}
        for r in base:
            first.setdefault(r[1], r[0])
        sweep = record(v for c in first.values() for v in dc.variants(c))
    records += base + sweep
    for opt in sorted({r[0].optimizer for r in base}):
        commits[opt] = a.commit
    missing = set(ENTRIES) - {r[1] for r in records}
    assert not missing, sorted(missing)
    assert {r[1] for r in records} <= set(ENTRIES), sorted({r[1] for r in records} - set(ENTRIES))
    entries = dc.pack(records)
    assert sorted(map(repr, dc.unpack(entries))) == sorted(map(repr, records))
    text = json.dumps({"recorded_from": commits, "shape": dict(rows=dc.ROWS, dim=dc.DIM, bags=dc.BAGS, nnz=dc.NNZ),
                       "cases": len(records), "entries": entries}, separators=(",", ":"))
    text = text.replace('},"ce_', '},\n"ce_').replace('"entries":{', '"entries":{\n') + "\n"
    assert len(text) < MAX_BYTES, len(text)
    Path(a.out).write_text(text)
    print(f"wrote {a.out}: {len(records)} cases ({len(base)} + {len(sweep)} of the sweep; {refused} refused before the "
          f"forward), {len(entries)} entries, {len(text)} bytes")


if __name__ == "__main__":
    main()
