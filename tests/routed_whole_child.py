"""Child process of test_gpu_routed_whole.py::test_routed_one_call_on_poisoned_memory, started with V2P_DEBUG_POISON=1 (every device
buffer filled with 0xA5 when allocated, read once per process).  argv[1]: a directory holding C4.npy and C5.npy, the oracle's digest
of every haplotype.  C4 and C5 whole through the one call; every digest after the first execute and after a re-execute over a
scribbled arena.  The last line of stdout is the sha256 of C5's whole BGZF output."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from whole_util import workers  # noqa: E402


def main(where):
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Context
    assert os.environ.get("V2P_DEBUG_POISON") == "1"
    sha = None
    with Context(0) as ctx:
        for preset, kernel in (("C4", 6), ("C5", 9)):
            want = np.load(os.path.join(where, f"{preset}.npy"))
            c = Cohort.preset(preset)
            n = c.n_haplotypes
            ctx.upload_proteome(c.proteome())
            stream = c.txstream(0, n, n_threads=workers())
            rs = ctx.upload_stream(stream)
            stream.close()
            b = ctx.batch()
            b.build_and_execute(rs, 0, 0)
            b.sync()
            assert b.oneshot_info()["kernel"] == kernel, (preset, b.oneshot_info(), b.image_form())
            for what in ("first execute", "re-execute"):
                got = np.asarray(b.digests(), dtype=np.uint64)
                bad = np.nonzero(got != want)[0]
                assert got.size == want.size and bad.size == 0, (preset, what, bad[:10])
                print(preset, what, "every digest is the oracle's", flush=True)
                if what == "first execute":
                    b.scribble(0x5A)
                    b.execute()
                    b.sync()
            if preset == "C5":
                total = b.bgzf()
                sha = hashlib.sha256(b.bgzf_download(0, total)).hexdigest()
            b.scribble()
            b.close()
            rs.close()
    print("sha256 C5", sha, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
