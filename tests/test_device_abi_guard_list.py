"""Every entry point of include/bppp.h that takes device memory - a `d_*` parameter, or a name that ends in `_device` (the block and mixed calls take
their HBM pointers inside a struct) - is a key of CASES in tests/test_gpu_guarded_outputs.py, which runs it with every device buffer inside a
GuardArena, or is listed in EXEMPT below with the reason it needs no such case.  An entry point added later fails here until it gets a guarded case.
The table is read from the source (no import: this runs where no GPU is), and every test it names must exist there and end in covered(), the
assertion that the named entry points were really called through the arena."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARDED = os.path.join(ROOT, "tests", "test_gpu_guarded_outputs.py")
MAX_EXEMPT = 6

EXEMPT = {
    "bppp_basis_create_device": "creates a handle, writes no caller buffer: it copies the points into HBM of its own (the handle's MSM is guarded as bppp_msm_basis)",
    "bppp_device_alloc": "its d_ptr is a host variable that receives the new allocation's address; no device buffer of the caller exists yet",
    "bppp_device_free":"releases an allocation of bppp_device_alloc, writes no caller buffer: the arena itself is freed through it",
    "bppp_rp_verify_shard_device": "multi-rank, covered by its single-rank twin: bppp_rp_verify_batch_device is this call with index_offset = 0",
    "bppp_rp_verify_shard_pub_device": "multi-rank, covered by its single-rank twin: bppp_rp_verify_batch_pub_device is this call with index_offset = 0",
}


def device_entry_points(header_text):
    """the bppp_* functions declared with a d_* parameter or named *_device"""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    found = set()
    for m in re.finditer(r"\b(bppp_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        name, params = m.group(1), m.group(2)
        if re.search(r"\bd_\w+", params) or name.endswith("_device"):
            found.add(name)
    return found


def case_table():
    """(CASES of the guarded tests as a dict, the test functions of that file -> their source)"""
    src = open(GUARDED).read()
    tree = ast.parse(src)
    table = next(ast.literal_eval(node.value) for node in tree.body
                 if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "CASES" for t in node.targets))
    tests = {node.name: ast.get_source_segment(src, node) for node in tree.body if isinstance(node, ast.FunctionDef) and node.name.startswith("test_")}
    return table, tests


def unguarded(entry_points, table, exempt):
    return sorted(entry_points - set(table) - set(exempt))


def test_the_scan_finds_the_entry_points_it_is_about():
    found = device_entry_points(open(os.path.join(ROOT, "include", "bppp.h")).read())
    assert {"bppp_msm_device", "bppp_msm_basis", "bppp_rp_cut_through_device", "bppp_rp_verify_block_device", "bppp_rp_verify_mixed_device", "bppp_upload",
            "bppp_rp_scan_keys_device", "bppp_points_from_seed_device", "bppp_rp_excess_halfagg_device"} <= found
    assert not {"bppp_msm", "bppp_rp_verify_batch", "bppp_host_alloc", "bppp_ctx_create", "bppp_rp_cut_through"} & found
    assert len(found) >= 60
    # a declaration the header does not have yet
    later = "int bppp_rp_new_thing_device(bppp_rp *rp, size_t n, const void *d_in, void *d_out);\nint bppp_other(bppp_ctx *ctx, void *d_buf);\nint bppp_host_only(int *x);"
    assert device_entry_points(later) == {"bppp_rp_new_thing_device", "bppp_other"}


def test_every_device_entry_point_has_a_guarded_case_or_a_stated_exemption():
    found = device_entry_points(open(os.path.join(ROOT, "include", "bppp.h")).read())
    table, tests = case_table()
    assert unguarded(found, table, EXEMPT) == [], "no guarded case: add one to tests/test_gpu_guarded_outputs.py and name it in CASES"
    assert len(EXEMPT) <= MAX_EXEMPT and all(reason.strip() for reason in EXEMPT.values())
    assert not set(EXEMPT) & set(table), "both guarded and exempt"
    assert not (set(table) | set(EXEMPT)) - found, "no such device entry point in include/bppp.h: %s" % sorted((set(table) | set(EXEMPT)) - found)
    # the table cannot claim more than the tests do: every test it names exists, is a gpu test of that file, and ends in covered() under its own name
    for fn, test in table.items():
        assert test in tests, "%s: no test %s" % (fn, test)
        assert re.search(r'covered\([^\n]*"%s"\)' % re.escape(test), tests[test]), "%s does not assert that its entry points were called" % test
    assert "pytestmark = pytest.mark.gpu" in open(GUARDED).read()


def test_one_case_less_and_one_declaration_more_are_noticed():
    found = device_entry_points(open(os.path.join(ROOT, "include", "bppp.h")).read())
    table, _ = case_table()
    for fn in table:                                               # removing any one case leaves that entry point unguarded
        assert unguarded(found, {k: v for k, v in table.items() if k != fn}, EXEMPT) == [fn]
    assert unguarded(found | {"bppp_rp_new_thing_device"}, table, EXEMPT) == ["bppp_rp_new_thing_device"]
