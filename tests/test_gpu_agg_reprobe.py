"""ngz_agg_push under a narrow key hash with MANY records per key: the exact re-probe of collided keys
(k_agg_reprobe, netgauze_amd/csrc/ngz_agg.hip) must not split a group when several records of one key
re-probe together.  A claimed slot showed its tag before its key was written, so a second record of
the key, finding the tag but not yet the key, claimed another slot: 40 keys came out as 115 groups
under a 4-bit hash.  (tests/test_gpu_agg.py's collision test has about one record per key.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agg_enrich_ref as AE  # noqa: E402
import ngz_agg_oracle as A  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = [(10, 4), (14, 4), (82, 16), (1, 8)]


@pytest.mark.parametrize("owner", [0, 1])
@pytest.mark.parametrize("bits,keys,n", [(4, 40, 400), (1, 7, 1000), (3, 300, 3000)])
def test_plain_push_keeps_groups_whole_under_a_narrow_hash(bits, keys, n, owner):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd import _lib
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    recs = [AE.record(T, (9, i % keys, ("if-%d" % (i % keys)).encode().ljust(16, b"\0"), 1 + i)) for i in range(n)]
    dgrams = [AE.template_msg(10, [(300, T)])] + [AE.data_msg(10, 300, recs[i:i + 256], seq=1 + i) for i in range(0, n, 256)]
    fields = [(0, 14, 0, 0), (0, 82, 0, 0), (0, 1, 0, 1)]
    agg = FlowAggregator(fields, options={_lib.NGZ_AGG_OPT_HASH_BITS: bits, _lib.NGZ_AGG_OPT_OWNER: owner}, capacity=1 << 12)
    agg.push(FlowInfoCodec(0, specialize=False).decode_datagrams(dgrams), 4739, 5)
    assert agg.last_path() == "general"
    got = sorted(AE.group_tuple(g) for g in agg.flush())
    ref = sorted(AE.group_tuple(g) for g in A.aggregate_datagrams(fields, dgrams, collection_ms=5).flush())
    assert len(got) == len(ref) == keys and got == ref
