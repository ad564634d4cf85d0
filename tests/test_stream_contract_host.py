"""Every prototype of include/tristage.h that takes a stream is classified in tests/stream_order.py (its kind, the
header sentence the kind rests on, the GPU case that holds it to it) or carries a written exemption.  A new entry
point fails here until it is classified.  No GPU."""
import os
import re

import stream_order as so

GPU_TESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_stream_order_gpu.py")


def _case_names():
    """The cases the GPU module defines: ``@case("name")`` builders and ``def test_<name>`` functions."""
    src = open(GPU_TESTS).read()
    names = set(re.findall(r'^@case\("(\w+)"', src, flags=re.M))
    names |= set(re.findall(r"^def test_(\w+)\(", src, flags=re.M))
    for m in re.finditer(r'^@pytest\.mark\.parametrize\("variant", \[([^\]]*)\]\)\ndef test_(\w+)\(', src, flags=re.M):
        names |= {f"{m.group(2)}_{v}" for v in re.findall(r'"(\w+)"', m.group(1))}
    return names


def test_the_header_has_about_fifty_stream_prototypes():
    protos = so.stream_prototypes()
    assert len(protos) == len(set(protos))
    assert 45 <= len(protos) <= 60, protos
    for name in ("ts_index_search", "ts_index_finish", "ts_group_topk", "ts_mlp_add_layernorm", "ts_compact_ivf",
                 "ts_bm25_search_batch_filtered", "ts_maxsim_passages_indexed_batch"):
        assert name in protos
    for name in ("ts_index_create", "ts_ivf_reset", "ts_index_last_ticket", "ts_bm25_set_index"):
        assert name not in protos


def test_every_stream_prototype_is_classified_or_exempt():
    assert so.table_problems(case_names=_case_names()) == []
    assert "ts_index_read_probe" in so.EXEMPT and len(so.EXEMPT) <= so.MAX_EXEMPT


def test_a_missing_row_is_noticed():
    for name in ("ts_index_mmr", "ts_geglu", "ts_update_ivf"):
        cut = {k: v for k, v in so.CONTRACT.items() if k != name}
        bad = so.table_problems(contract=cut, case_names=_case_names())
        assert len(bad) == 1 and bad[0].startswith(name + ":"), bad


def test_a_new_entry_point_is_noticed():
    header = so.header_text().replace("int ts_abi_version(void);",
                                      "int ts_new_call(const float* x,\n                void* stream);\nint ts_abi_version(void);")
    bad = so.table_problems(header=header, case_names=_case_names())
    assert bad == ["ts_new_call: takes a stream and is neither classified nor exempt"]


def test_rows_are_held_to_the_header_and_to_the_gpu_cases():
    row = so.CONTRACT["ts_index_mmr"]
    for broken, word in (((row[0], "the call returns at once, honestly", row[2]), "sentence"),
                         (("eventually", row[1], row[2]), "kind"),
                         ((row[0], row[1], "no_such_case"), "covering case"),
                         ((row[0], row[1], ""), "covering case")):
        bad = so.table_problems(contract=dict(so.CONTRACT, ts_index_mmr=broken), case_names=_case_names())
        assert len(bad) == 1 and word in bad[0], bad
    many = dict(so.EXEMPT)
    moved = dict(so.CONTRACT)
    for name in list(so.CONTRACT)[: so.MAX_EXEMPT]:
        many[name] = "moved out of the table to see whether that is noticed"
        del moved[name]
    assert any("exemptions" in b for b in so.table_problems(contract=moved, exempt=many, case_names=_case_names()))
    assert any("written reason" in b for b in so.table_problems(exempt={"ts_index_read_probe": "no"}, case_names=_case_names()))


def test_the_delay_is_within_the_bounds_of_the_probe():
    import json
    probe = json.load(open(os.path.join(so.ROOT, "profiles", "stream_order_probe.json")))
    slowest = max(probe["enqueue_host_ms"].values())
    assert probe["delay_ms_chosen"] == so.DELAY_MS
    assert 10.0 * slowest <= so.DELAY_MS <= so.DELAY_MAX_MS, (slowest, so.DELAY_MS)
