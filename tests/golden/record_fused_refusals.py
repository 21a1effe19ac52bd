"""Records tests/golden/fused_refusals.json: what the fused-update switches' constructors (stage A), the set_fused_*
setters (stage B) and the front of embedding_bag (stage C) of the checkout given by --repo answer to the cases of
tests/fused_refusal_cases.py.

    python tests/golden/record_fused_refusals.py --part cpu --repo <checkout with its own build> --commit <its hash>
    python tests/golden/record_fused_refusals.py --part gpu --repo <the same checkout> --commit <its hash>

`cpu` records the three stages on CPU tensors and needs no GPU.  `gpu` records gpu_cases() -- the stage-C cases whose
switch keeps state on the device -- with every tensor on the GPU; no kernel runs there either.  Either part is merged
into the fixture that is already there.  The fixture holds two base-62 digits per case: an index into `answers`, the
distinct (exception class | "reached" | "accepted", message) pairs; stage B holds a second index per case, into `states`,
the digests of the switches' fields after the call.
The fixture in the repository was recorded from the parent of the commit that gave the refusals one rule set:
regenerating it from the code it checks would prove nothing."""
import argparse
import ast
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
MAX_BYTES = 200 * 1024
# literals of the front that no call can reach: check_lr refuses a tensor of more than one element first, and one
# element is contiguous whatever its strides
UNREACHABLE = ("a tensor learning rate must be contiguous",)
# where the front's refusals are written: the switches and the check helpers, the setters, the sharded module's setters
SCANNED = {"functional.py": ("check_", "refuse_", "Fused", "embedding_bag"),
           "cached_embedding.py": ("_checked_", "_refuse_", "set_fused_", "set_weight_rounding"),
           "parallel.py": ("RowwiseShardedEmbeddingBag.set_fused_",)}


def message_literals(repo: Path):
    """the longest literal fragment of every message the scanned functions raise (embedding_bag: up to its _prep call)"""
    out = []
    for name, prefixes in SCANNED.items():
        tree = ast.parse((repo / "cachedembedding_amd" / name).read_text())
        scopes = []
        for node in tree.body:
            if isinstance(node, ast.ClassDef):
                scopes += [(f"{node.name}.{f.name}", f) for f in node.body if isinstance(f, ast.FunctionDef)]
                scopes.append((node.name, None))
            elif isinstance(node, ast.FunctionDef):
                scopes.append((node.name, node))
        for qual, fn in scopes:
            if fn is None or not (qual.startswith(prefixes) or qual.split(".")[-1].startswith(prefixes)):
                continue
            stop = min((n.lineno for n in ast.walk(fn) if isinstance(n, ast.Call) and
                        getattr(n.func, "id", "") == "_prep"), default=1 << 30)
            for r in ast.walk(fn):
                if isinstance(r, ast.Raise) and r.exc is not None and r.lineno < stop:
                    parts = [c.value for c in ast.walk(r.exc) if isinstance(c, ast.Constant) and isinstance(c.value, str)]
                    if parts:
                        out.append((f"{name}:{qual}", max(parts, key=len)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["cpu", "gpu"])
    ap.add_argument("--repo", default=str(HERE.parent.parent))
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=str(HERE / "fused_refusals.json"))
    a = ap.parse_args()
    sys.path.insert(0, a.repo)                        # the package under test
    sys.path.insert(1, str(HERE.parent))              # the case generator
    import torch

    import cachedembedding_amd as ce
    import fused_refusal_cases as fc
    from cachedembedding_amd import functional as F
    from cachedembedding_amd.parallel import RowwiseShardedEmbeddingBag
    repo = Path(a.repo).resolve()
    assert Path(ce.__file__).resolve().is_relative_to(repo)
    out = Path(a.out)
    fix = json.loads(out.read_text()) if out.exists() else {"answers": [], "states": [], "cases": {}}
    assert fix.setdefault("commit", a.commit) == a.commit, "the fixture holds answers of another commit"
    answers = fix["answers"]
    lookup = {tuple(x): i for i, x in enumerate(answers)}

    def index(rows):
        for r in rows:
            if r not in lookup:
                lookup[r] = len(answers)
                answers.append(list(r))
        return fc.encode([lookup[r] for r in rows])

    def both(rows, stage):
        kinds = {k in ("accepted", "reached") for k, _ in rows}
        assert kinds == {True, False}, f"stage {stage} needs refused and accepted cases"

    if a.part == "cpu":
        rows_a = fc.brief_outcomes(fc.run_stage_a(F))
        rows_b = fc.brief_states(fc.run_stage_b(F, ce.CachedEmbeddingBag, RowwiseShardedEmbeddingBag))
        cases_c = fc.stage_c_cases()
        rows_c = fc.run_stage_c(F, cases_c)
        both(rows_a, "A"), both([r for r, _ in rows_b], "B"), both(rows_c, "C")
        fix["a"], fix["b"], fix["c"] = index(rows_a), index([r for r, _ in rows_b]), index(rows_c)
        fix["states"] = sorted({s for _, s in rows_b})
        fix["b_state"] = fc.encode([fix["states"].index(s) for _, s in rows_b])
        fix["cases"].update(a=[len(rows_a), fc.digest(fc.stage_a_cases())], b=[len(rows_b), fc.digest(fc.stage_b_cases())],
                            c=[len(rows_c), fc.digest(cases_c)])
        print("stage A:", len(rows_a), "cases; stage B:", len(rows_b), "cases,", len(fix["states"]), "states; stage C:",
              len(rows_c), "cases")
    else:
        assert torch.cuda.is_available(), "the GPU column is recorded with the tensors on the device"
        cases = fc.gpu_cases()
        rows = fc.run_stage_c(F, cases, torch.device("cuda", torch.cuda.current_device()))
        both(rows, "C on the GPU")
        fix["gpu"] = index(rows)
        fix["cases"]["gpu"] = [len(rows), fc.digest(cases)]
        print("GPU column:", len(rows), "cases")
    if all(k in fix for k in ("a", "b", "c", "gpu")):
        said = [msg for _, msg in answers]
        missing = [(where, lit) for where, lit in message_literals(repo)
                   if lit not in UNREACHABLE and not any(lit in m for m in said)]
        assert not missing, f"no case produces these messages of the front: {missing}"
    text = json.dumps(fix, separators=(",", ":")).replace('],["', '],\n["') + "\n"
    assert len(text) < MAX_BYTES, len(text)
    out.write_text(text)
    print("wrote", out, len(text), "bytes,", len(answers), "distinct answers")


if __name__ == "__main__":
    main()
