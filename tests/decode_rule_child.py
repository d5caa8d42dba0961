"""Child process of test_gpu_decode_rule.py::test_product_cases_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device buffer
filled with 0xA5 when allocated, read once per process): the seam cases that are whole VCFs once more through the product call, every
list equal to the rule's.  A kernel that read what it had not written (the carrier rows past row_nnz, the counts, the side list) would
show here.  Prints one line per case; the last line is "decode rule child ok"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import decode_rule as R  # noqa: E402
from test_gpu_decode_rule import assert_product  # noqa: E402


def main():
    from vcf2prot_amd.engine import Context
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    with Context(0) as ctx:
        for case in R.product_cases():
            assert_product(ctx, case)
            want = case.want()
            print(case.name, want if isinstance(want, tuple) else sum(map(len, want)), flush=True)
    print("decode rule child ok", flush=True)


if __name__ == "__main__":
    main()
