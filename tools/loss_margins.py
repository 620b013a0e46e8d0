"""profiles/loss_family_margins.json from the records of tests/test_gpu_loss.py.

Every test of that module records its largest error / bound through tests/conftest.py: record_parity as a line
{"test": "loss_family:<entry>/<kind>", "ratio": r} of the parity record file.  This merges such a file into the table
{key: largest ratio seen}: keys already in the table keep the larger value, new keys are added.

    python tools/loss_margins.py <parity_errors.jsonl> [profiles/loss_family_margins.json]
"""
import json
import os
import sys

PREFIX = "loss_family:"


def merge(records_path, table_path):
    table = json.load(open(table_path)) if os.path.exists(table_path) else {}
    for line in open(records_path):
        rec = json.loads(line)
        if rec.get("test", "").startswith(PREFIX):
            key = rec["test"][len(PREFIX):]
            table[key] = max(float(rec["ratio"]), table.get(key, 0.0))
    with open(table_path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    return table


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "profiles", "loss_family_margins.json")
    t = merge(sys.argv[1], out)
    print(f"{len(t)} keys, largest ratio {max(t.values()):.3f}")
