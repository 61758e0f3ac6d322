"""CPU: the Avro binary writer of tests/output_ref.py on hand-computed vectors (the Avro
specification's zigzag varints, length-prefixed strings, one-block arrays and unions)."""
import pytest

import output_ref as R


@pytest.mark.parametrize("v,want", [(0, "00"), (-1, "01"), (1, "02"), (63, "7e"), (64, "8001"), (-65, "8101"),
                                    (2**63 - 1, "feffffffffffffffff01"), (-2**63, "ffffffffffffffffff01")])
def test_long(v, want):
    assert R.w_long(v).hex() == want


def test_values_unions_and_arrays():
    assert R.w_value("string", "foo").hex() == "06666f6f"
    assert R.w_value("bytes", b"\x00\xff").hex() == "0400ff"
    assert R.w_value("array", []).hex() == "00"
    assert R.w_value("array", ["a", "bc"]).hex() == "04026104626300"
    assert R.w_value("boolean", True).hex() == "01" and R.w_value("float", 0x3FC00000).hex() == "0000c03f"
    assert R.w_field(None, True).hex() == "00"
    assert R.w_field(("long", 3), True).hex() == "0206" and R.w_field(("long", 3), False).hex() == "06"


def test_a_u64_past_i64_goes_negative_and_fields_follow_config_order():
    import ngz_oracle as O
    f = lambda ie, v: O.Field(O.REGISTRY.lookup(0, ie), v)  # noqa: E731
    rec = [f(1, 2**63), f(8, ("v4", 0x0A000001)), f(1, 5)]
    cfg = [{"name": "b1", "refs": [(0, 1, 1)]}, {"name": "b0", "refs": [(0, 1, 0)]},
           {"name": "ip", "refs": [(0, 12, 0), (0, 8, 0)], "select": "Coalesce", "transform": "String"},
           {"name": "p", "refs": [(0, 2, 0)], "default": ("U64", 2**64 - 1)}, {"name": "n", "refs": [(0, 2, 0)]}]
    assert R.datum(cfg, rec).hex() == "020a" + "02" + R.w_long(-2**63).hex() + "02" + "1031302e302e302e31" + "01" + "00"
