"""Child process of test_gpu_tasks_rule.py::test_cases_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device buffer filled
with 0xA5 when allocated, read once per process): the seam cases, the deep group and the seeded groups once more, every array of the
stream equal to the rule's.  A kernel that read memory it had not written (the counts, the kinds, the prefix sums, the slack behind the
Task arrays) would show here.  Prints one line per case; the last line is "tasks rule child ok"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import tasks_rule as T  # noqa: E402
from test_gpu_tasks_rule import run_case  # noqa: E402


def main():
    from vcf2prot_amd.engine import Context
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    with Context(0) as ctx:
        for case in [T.case_items(n) for n in (1, 64, 257)] + [T.case_deep_and_edges(), T.case_seeded_groups(400)]:
            rules = run_case(ctx, T.without_aborts(case))
            print(case.name, [sum(r.per_hap()[0]) for r in rules], flush=True)
    print("tasks rule child ok", flush=True)


if __name__ == "__main__":
    main()
