"""Every C ABI entry point that takes a Krylov state settles a pending close first, unless it is on the list of those that may not.

A batch of one-sweep Lanczos steps leaves its newest column unwritten (library.hip: StepCursor::close_pending, settle_columns).
The rule is an allow-list, so that a new entry point is safe by default: this test reads the header for every function with an
eigenex_basis_t argument and the library source for its body, and fails for one that neither calls enter_settled (itself or
through the helper it hands the state to) nor is listed here and in the comment in front of the C ABI.  No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "eigenex_hip.h")
LIBRARY = os.path.join(ROOT, "cmpt-eigenex_amd", "csrc", "library.hip")

DOES_NOT_SETTLE = {
    "eigenex_lanczos_state", "eigenex_basis_repairs", "eigenex_basis_configure", "eigenex_basis_configure_z",
    "eigenex_basis_set_alpha_fusion", "eigenex_basis_capacity", "eigenex_basis_is_complex", "eigenex_basis_graph_info",
    "eigenex_basis_close_pending", "eigenex_basis_clear", "eigenex_basis_destroy",
}
SETTLES_CONDITIONALLY = {"eigenex_lanczos_enqueue": "sweeps_once(b)"}  # not when a one-sweep step follows


def _entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = []
    for m in re.finditer(r"\bint\s+(eigenex_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\beigenex_basis_t\s+\w+", m.group(2)):  # a state handed in (eigenex_basis_t* out: one handed back)
            out.append(m.group(1))
    return out


def _bodies():
    text = open(LIBRARY).read()
    bodies = {}
    for m in re.finditer(r"^(?:static\s+)?int\s+(\w+)\s*\([^;{]*?\)\s*\{", text, flags=re.M | re.S):
        eol = text.index("\n", m.end())
        one_line = text[m.end():eol].rstrip().endswith("}")
        bodies[m.group(1)] = text[m.end():eol if one_line else text.index("\n}\n", eol)]
    return bodies


def _settles(name, bodies, depth=0):
    body = bodies[name]
    if "enter_settled(" in body:
        return True
    if depth == 2:
        return False
    return any(callee != name and callee in bodies and _settles(callee, bodies, depth + 1) for callee in set(re.findall(r"\b(\w+)\s*\(", body)))


def test_every_entry_point_with_a_state_settles_or_is_listed():
    names, bodies = _entry_points(), _bodies()
    assert len(names) > 30 and "eigenex_vec_download" in names and "eigenex_spin_site_apply" in names
    missing = [n for n in names if n not in bodies]
    assert not missing, "no definition found for %s" % missing
    unsettled = [n for n in names if n not in DOES_NOT_SETTLE and not _settles(n, bodies)]
    assert not unsettled, "these take a state and neither settle it nor are listed as exempt: %s" % unsettled
    for n in DOES_NOT_SETTLE:
        assert n in names and "enter_settled(" not in bodies[n], n
    for n, cond in SETTLES_CONDITIONALLY.items():
        assert cond in bodies[n] and "enter_settled(" in bodies[n]


def test_the_list_in_the_source_names_the_same_entry_points():
    text = open(LIBRARY).read()
    block = text[text.index("takes a state calls enter_settled first, EXCEPT"):text.index("A new entry point is not on the list")]
    listed = set(re.findall(r"\beigenex_\w+", block.replace("configure[_z]", "configure eigenex_basis_configure_z")))
    assert listed == DOES_NOT_SETTLE | set(SETTLES_CONDITIONALLY)
