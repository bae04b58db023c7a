"""-m "not gpu": the host side of the C ABI answers exactly what tests/golden/abi_table.json recorded -- every plan, workspace size and
support answer as the same integers, every refusal with the same return code and the same error string, character for character, every call that has nothing
to do with HYD_OK, every accepted call with the name of the launch it reaches first.
The table was recorded (python tests/abi_table.py --write) from the parent of the last change to csrc/api_*.hip; it is data, and
is not regenerated from the code it checks."""
import pytest

from tests import abi_table


@pytest.fixture(scope="module")
def table():
    return abi_table.load_fixture()


def test_table_and_case_list_are_the_same_set(table):
    ids = [c[0] for c in abi_table.QUERY_CASES + abi_table.REFUSAL_CASES + abi_table.NOOP_CASES + abi_table.LAUNCH_CASES]
    assert sorted(ids) == sorted(table)
    assert all(rec["rc"] not in (abi_table.HYD_OK, abi_table.HYD_ERR_LAUNCH) for cid, rec in table.items() if cid.startswith("refusal:"))
    assert all(rec == {"rc": abi_table.HYD_OK} for cid, rec in table.items() if cid.startswith("noop:"))
    launches = [rec for cid, rec in table.items() if cid.startswith("launch:")]
    assert launches and all(set(rec) == {"rc", "what"} and rec["rc"] == abi_table.HYD_ERR_LAUNCH and rec["what"] for rec in launches)


def test_shapes_only_queries_match_the_record(table):
    wrong = {}
    for case in abi_table.QUERY_CASES:
        got = abi_table.run_case(case)
        if got != table[case[0]]:
            wrong[case[0]] = (got, table[case[0]])
    assert not wrong, f"{len(wrong)} of {len(abi_table.QUERY_CASES)} differ (got, recorded): {dict(list(wrong.items())[:5])}"


def test_refusals_match_the_record(table):
    """Runs only without a device: a refusal that a regression turns into an acceptance would launch a kernel on made-up addresses;
    without a device the same regression comes back as HYD_ERR_LAUNCH instead of the recorded code."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("refusals are replayed on machines without a device only")
    wrong = {}
    for case in abi_table.REFUSAL_CASES:
        got = abi_table.run_case(case)
        if got != table[case[0]]:
            wrong[case[0]] = (got, table[case[0]])
    assert not wrong, f"{len(wrong)} of {len(abi_table.REFUSAL_CASES)} differ (got, recorded): {dict(list(wrong.items())[:5])}"


def test_launches_match_the_record(table):
    """Accepted calls reach the launch the parent reached: without a device that launch answers HYD_ERR_LAUNCH under its own name.
    Runs only without a device: with one, every case would run a kernel on made-up addresses."""
    if abi_table.device_present():
        pytest.skip("accepted calls are replayed on machines without a device only")
    wrong = {}
    for case in abi_table.LAUNCH_CASES:
        got = abi_table.run_case(case)
        if got != table[case[0]]:
            wrong[case[0]] = (got, table[case[0]])
    assert not wrong, f"{len(wrong)} of {len(abi_table.LAUNCH_CASES)} differ (got, recorded): {dict(list(wrong.items())[:5])}"


@pytest.mark.parametrize("entry, kw", [
    ("hyd_decode_attn_fused", {"kv_len": 1 << 20, "suffix.k_tok_stride": 1024}),
    ("hyd_decode_attn_fused", {"Hq": 4 * 65535 + 1, "Hkv": 4 * 65535 + 1}),
    ("hyd_decode_attn_fused_kvq", {"kq": {}, "kv_len": 1 << 20, "suffix.k_tok_stride": 2048}),
])
def test_unique_pass_limits_are_refused_before_the_level_passes(table, entry, kw):
    """What the unique pass refuses (a sequence's K/V span, the grid limits) is known from the shapes: HYD_PHASE_ALL answers it before
    its level passes go out, with the code and the words HYD_PHASE_UNIQUE has in the record."""
    if abi_table.device_present():
        pytest.skip("a regression would launch on made-up addresses")
    lib = abi_table._lib.load()
    recorded = table[abi_table._case_id("refusal", entry, {"phase": abi_table._lib.HYD_PHASE_UNIQUE, **kw})]
    assert abi_table.REFUSALS[entry](lib, {"phase": abi_table._lib.HYD_PHASE_ALL, **kw}) == recorded


def test_noops_match_the_record(table):
    """Calls that return HYD_OK before any HIP call.  Runs only without a device, like the refusals: a regression that launches comes
    back as HYD_ERR_LAUNCH there instead of the recorded HYD_OK, and would run a kernel on made-up addresses where a device is."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("no-op calls are replayed on machines without a device only")
    wrong = {}
    for case in abi_table.NOOP_CASES:
        got = abi_table.run_case(case)
        if got != table[case[0]]:
            wrong[case[0]] = (got, table[case[0]], abi_table._lib.load().hyd_last_error_string().decode())
    assert not wrong, f"{len(wrong)} of {len(abi_table.NOOP_CASES)} differ (got, recorded, last error): {wrong}"
