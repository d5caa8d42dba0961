"""Child process of test_gpu_stats_rule.py::test_large_cases_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device buffer filled
with 0xA5 when allocated, read once per process): the large synthetic cases once more, every table equal to the rule's.  A kernel that
counted on memory it had not written (the LDS bins and bitmaps, the tables, the status words) would show here.  Prints one line per
case; the last line is "stats rule child ok"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import stats_rule as R  # noqa: E402
from test_gpu_stats_rule import LARGE, assert_kernel_equals_rule, decoded  # noqa: E402


def main():
    from vcf2prot_amd.engine import Context
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    with Context(0) as ctx:
        for name, make in list(LARGE.items()) + [("long_list", R.case_long_list), ("capacity_8192", lambda: R.case_capacity(8192))]:
            case = make()
            with decoded(ctx, case) as res:
                for caps in {"long_list": (None, (0, 8192, 2048)), "capacity_8192": ((0, 0, 16384), (0, 1, 16384))}.get(name, (None, (0, 1, 16384))):
                    info = assert_kernel_equals_rule(ctx, res, case, caps)
                    print(name, caps, info["lds_bytes"], info["n_sorted_members"], flush=True)
    print("stats rule child ok", flush=True)


if __name__ == "__main__":
    main()
