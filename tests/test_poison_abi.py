"""The poison hooks (bppp_test_ctx_poison, bppp_test_rp_poison: include/bppp_test.h) are declared, live in the test library only, are typed in capi.py and
refuse NULL; and every pointer member of bppp_ctx (csrc/ctx.hpp) and bppp_rp (csrc/rp_internal.hpp) is classified: filled by its hook in
csrc/testhooks.hip, or listed in PERSISTENT below with the reason it is not scratch.  A buffer added later fails the completeness check until someone
decides which of the two it is."""
import ctypes as C
import os
import re

from bulletproofspp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bulletproofspp_amd", "csrc")
ERR_ARG = -1
HOOKS = ("bppp_test_ctx_poison", "bppp_test_rp_poison")

# pointer members that the hooks leave alone: struct -> member -> why it is not scratch
PERSISTENT = {
    "bppp_ctx": {
        "pre_acc": "not a buffer: the one-shot upload hook of bppp_msm, set and cleared within one call",
        "pre_acc_arg": "not a buffer: the argument of pre_acc",
    },
    "bppp_rp": {
        "ctx": "the handle's context; the caller poisons it with bppp_test_ctx_poison",
        "twin": "the twin handle; the hook recurses into it",
        "twin_ctx": "the twin's context; the hook poisons it through the context's own routine",
        "pool": "host worker threads of the host oracle, not a buffer",
        "btabs": "device tables of a binary setup, uploaded at creation",
        "tabs": "device tables of a typed setup, uploaded at creation",
        "d_basis": "the basis [g | H | G], uploaded at creation",
        "d_plan": "the hash plan, uploaded at creation",
        "d_fixed": "window table of (g, H0, H1), built once at first use",
        "commit_basis": "registered basis with its table, built once at first use",
        "comb": "the comb table, built once (or shared) and read by every later prove",
        "d_wit": "per-range data of the witness kernels, uploaded at the first device prove",
        "pre_inputs": "borrowed: the caller's input commitments while bppp_rp_prove_mixed runs",
    },
}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _braces(text, start):
    """the text between the brace at or after `start` and its partner"""
    i = text.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
        j += 1


def _strip_nested(body):
    out, depth = [], 0
    for ch in body:
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif depth == 0:
            out.append(ch)
    return "".join(out)


def pointer_members(path, struct):
    text = re.sub(r"//[^\n]*", "", open(path).read())
    body = _strip_nested(_braces(text, re.search(r"\bstruct\s+%s\s*\{" % struct, text).start()))
    names = []
    for stmt in body.split(";"):
        for m in re.finditer(r"\*\s*(\w+)\s*(\(?)", stmt):
            if m.group(1) != "const" and not m.group(2):         # a data member, not a method that returns a pointer
                names.append(m.group(1))
    return names


def poisoned_members(func, handle):
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "testhooks.hip")).read())
    body = _braces(text, re.search(r"\bint\s+%s\s*\(" % func, text).start())
    return set(re.findall(r"P\.(?:hbm|host)\(%s->(\w+)" % handle, body))


def test_hooks_are_declared_typed_and_in_the_test_library_only():
    lib, tlib = capi.load_library(), capi.load_test_library()
    for name in HOOKS:
        assert re.search(r"\b%s\s*\(" % name, _header("bppp_test.h"))
        assert not re.search(r"\b%s\b" % name, _header("bppp.h"))
        assert hasattr(tlib, name) and not hasattr(lib, name)
        assert name not in capi.SYMBOLS
        assert len(getattr(tlib, name).argtypes) == 3


def test_null_handle_is_an_argument_error():
    tlib = capi.load_test_library()
    n = C.c_uint64(7)
    assert tlib.bppp_test_ctx_poison(None, 0xA5, C.byref(n)) == ERR_ARG
    assert tlib.bppp_test_rp_poison(None, 0xA5, C.byref(n)) == ERR_ARG
    assert tlib.bppp_test_ctx_poison(None, 0, None) == ERR_ARG and tlib.bppp_test_rp_poison(None, 0, None) == ERR_ARG


def test_the_scan_finds_the_members_it_is_about():
    ctx, rp = pointer_members(os.path.join(CSRC, "ctx.hpp"), "bppp_ctx"), pointer_members(os.path.join(CSRC, "rp_internal.hpp"), "bppp_rp")
    assert {"ws", "ws2", "mix", "pinned", "pre_acc", "pre_acc_arg"} <= set(ctx)
    assert {"pwork", "awork", "work", "stage", "ework", "hpin", "hstage", "hflag", "d_pub", "d_sel", "d_bind", "d_bhdr", "d_comb_out", "d_basis", "d_plan", "twin",
            "comb"} <= set(rp)
    assert "d_g" not in rp and "d_H" not in rp                  # methods, not members
    assert len(ctx) == len(set(ctx)) and len(rp) == len(set(rp))


def test_every_pointer_member_is_poisoned_or_listed_as_persistent():
    cases = (("bppp_ctx", "ctx.hpp", "ctx_poison", "ctx"), ("bppp_rp", "rp_internal.hpp", "rp_poison", "rp"))
    for struct, header, func, handle in cases:
        members = set(pointer_members(os.path.join(CSRC, header), struct))
        filled, kept = poisoned_members(func, handle), set(PERSISTENT[struct])
        assert filled, f"{func} fills nothing"
        assert not (filled & kept), f"{struct}: both poisoned and listed as persistent: {sorted(filled & kept)}"
        assert not (members - filled - kept), f"{struct}: unclassified pointer members {sorted(members - filled - kept)}: poison them in {func} or list them in PERSISTENT"
        assert not ((filled | kept) - members), f"{struct}: no such pointer member: {sorted((filled | kept) - members)}"
        assert all(reason.strip() for reason in PERSISTENT[struct].values())
    assert poisoned_members("ctx_poison", "ctx") == {"ws", "ws2", "mix", "pinned"}
