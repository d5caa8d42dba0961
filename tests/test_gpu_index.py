"""GPU suite of the device-built record index on VCF files: on the golden VCFs, the decode cases and the random VCFs
(tests/index_rule.py::file_texts), flat, gzip-inflated on the host and as BGZF inflated on the device, the columns
v2p_decode_index_download hands out equal the host build's, and VcfIndex.from_device reads like VcfIndex."""
import gzip

import pytest

import index_rule as R
import inflate_corpus as C
from test_index_rule import columns_of, message_of

pytestmark = pytest.mark.gpu
TEXTS = R.file_texts()


@pytest.mark.parametrize("name,text", TEXTS, ids=[n for n, _ in TEXTS])
def test_device_columns_equal_host_columns(built, gpu_ctx, name, text):
    from vcf2prot_amd.frontend import VcfIndex, inflate_bgzf, input_format, upload_text
    raw = text.encode()
    host = VcfIndex(raw)
    want, names = columns_of(host), host.sample_names()
    z = gzip.compress(raw)
    assert input_format(z) == "gzip"
    bz = C.bgzf(raw, block=4000, level=6)
    text2, inflated = inflate_bgzf(gpu_ctx, bz)
    assert text2 == raw
    for form, body, resident in (("flat", raw, upload_text(gpu_ctx, raw)), ("gzip", gzip.decompress(z), None), ("bgzf", text2, inflated)):
        if resident is None:
            resident = upload_text(gpu_ctx, body)
        try:
            idx = VcfIndex.from_device(gpu_ctx, body, resident)
            assert idx.path == "device" and columns_of(idx) == want and idx.sample_names() == names, (name, form)
            assert idx.consequence(idx.n_consequences - 1) == host.consequence(host.n_consequences - 1)
            assert idx.record_of(idx.n_consequences - 1) == host.n_records - 1
            idx.close()
        finally:
            resident.close()
    host.close()


def test_a_malformed_file_is_refused_alike(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import VcfIndex, inflate_bgzf, upload_text
    for name, text in R.order_cases() + [("no_header", "1\t2\t3\t4\t5\t6\t7\t8\t9\t10\n")]:
        raw = text.encode()
        with pytest.raises(N.V2PError) as h:
            VcfIndex(raw)
        for resident in (upload_text(gpu_ctx, raw), inflate_bgzf(gpu_ctx, C.bgzf(raw))[1]):
            with pytest.raises(N.V2PError) as d:
                VcfIndex.from_device(gpu_ctx, raw, resident)
            resident.close()
            assert d.value.code == h.value.code == -26 and message_of(d.value) == message_of(h.value), name
            assert d.value.index == R.verdict_by_rule(text)[1].line
