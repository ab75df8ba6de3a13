"""The table of accel kinds (csrc/accel_kinds.h) against an independent statement of what the host code decided per kind before the table
existed: the predicates of accel.h and the kind lists of launch_on, service_trace, launch_cull and rtcamdGetSceneStats, written out here as
plain sets of kind numbers.  The library reports a row through rtcamdDebugAccelKindRow (rtc.accel_kind_row).  No GPU."""
KINDS = range(48)

# ---- the predicates of accel.h as they stood ------------------------------------------------------------------------------------------
CURVE = {42, 43}                                   # is_curve_kind
LINE = {36, 37}                                    # is_line_kind
INST_LINEAR = {30, 31}                             # is_inst_linear_kind
INST_TOP_LINEAR = {32, 33}                         # is_inst_top_linear_kind
INST_SUBDIV_TOP_LINEAR = {34, 35}                  # is_inst_subdiv_top_linear_kind
INST_TWO_SECTION = INST_LINEAR | INST_TOP_LINEAR | INST_SUBDIV_TOP_LINEAR  # is_inst_two_section_kind
INST_GENERAL = {22, 23} | INST_LINEAR | INST_TOP_LINEAR                    # is_inst_general_kind
INSTANCE = set(range(14, 26)) | INST_TWO_SECTION   # is_instance_kind
LINE_MB = set(range(38, 42))                       # is_line_mb_kind
CURVE_MB = set(range(44, 48))                      # is_curve_mb_kind
MB_LINEAR = set(range(26, 30)) | {40, 41, 46, 47}  # is_mb_linear_kind
MB_PLUECKER = {10, 12, 26, 28}                     # is_mb_pluecker_kind
MB_MESH = set(range(10, 14)) | MB_LINEAR | LINE_MB | CURVE_MB  # is_mb_mesh_kind

# ---- the kind lists of the call sites --------------------------------------------------------------------------------------------------
TRACED = set(range(1, 48))                         # every kind but ACCEL_NONE has a launcher
POOL_PAYS = {1, 2, 5}                              # launch_on: poolPays
POOL = TRACED - MB_MESH - CURVE - INSTANCE         # launch_on: the three clauses that switched the pool form off
CULL = TRACED - INSTANCE - MB_LINEAR - LINE - LINE_MB - CURVE - CURVE_MB  # launch_on: the seven negated predicates of the pre-pass
OCT_ALWAYS, OCT_QUAD_FORM = {6}, {3, 4, 7}         # launch_on: octOnly
OCT_LEAF_24 = {6}                                  # launch_on and service_trace: 24 for grid cells, else 16
SERVICE = TRACED - MB_MESH - INSTANCE - LINE - CURVE  # service_trace: its four deny clauses
SERVICE_KERNELS = set(range(1, 10))                # launch_service: the kinds its switch served
LEVEL_FREE = {1, 2, 8, 9, 6}                       # service_trace: levelFree
CULL_FAST = {2, 9, 11, 13}                         # launch_cull: robust unless one of these
PRIMS_IN_PRIMS = {1, 2}                            # rtcamdGetSceneStats: tri
INST_SUBDIV = {24, 25, 34, 35}                     # the subdivision instance accel (Scene::instSubdivAccel)
# launch_trace: the groups of its switch, one per launch_trace_*
LAUNCHERS = [{1, 2}, {8, 9}, {10, 11, 26, 27}, {12, 13, 28, 29}, {6}, {3}, {4}, {5}, {7}, {36, 37}, {38, 39, 40, 41}, {42, 43}, {44, 45, 46, 47},
             set(range(14, 22)), {22, 23}, {24, 25}, {30, 31}, {32, 33}, {34, 35}]
# the builders' Pluecker / robust choice, by the kinds' names: the odd one of each pair below is the robust one, every subdivision kind is robust
ROBUST = {1, 8, 10, 12, 14, 16, 18, 20, 22, 26, 28, 30, 32, 36, 38, 40, 42, 44, 46} | {3, 4, 5, 6, 7} | INST_SUBDIV


def _rows(rtc):
    return {k: rtc.accel_kind_row(k) for k in KINDS}


def _having(rows, field, value=1):
    return {k for k, r in rows.items() if r[field] == value}


def test_the_statement_is_consistent():
    """the deny lists of service_trace left exactly the kinds launch_service had a kernel for; launch_cull's list agrees with
    is_mb_pluecker_kind and with the builders' choice wherever the pre-pass could run"""
    assert SERVICE == SERVICE_KERNELS
    assert {k for k in MB_MESH if k < 30} - MB_PLUECKER == {11, 13, 27, 29}
    assert CULL - CULL_FAST == CULL & ROBUST and MB_PLUECKER <= ROBUST
    assert set().union(*LAUNCHERS) == TRACED and sum(len(v) for v in LAUNCHERS) == len(TRACED)


def test_every_kind_has_its_row(rtc):
    rows = _rows(rtc)
    assert all(r is not None for r in rows.values())
    for kinds in LAUNCHERS:  # a row names its launcher by the first kind that shares it
        assert _having(rows, "launcher", min(kinds)) == kinds
    assert _having(rows, "launcher", 0) == {0}
    assert _having(rows, "robust") == ROBUST
    assert _having(rows, "nodes", rtc.KIND_NODES.index("qnodemb8")) == MB_LINEAR
    assert _having(rows, "nodes", rtc.KIND_NODES.index("two_section")) == INST_TWO_SECTION
    assert _having(rows, "inst", rtc.KIND_INST.index("none")) == set(KINDS) - INSTANCE
    assert _having(rows, "inst", rtc.KIND_INST.index("subdiv")) == INST_SUBDIV
    assert _having(rows, "inst", rtc.KIND_INST.index("mesh")) == INSTANCE - INST_SUBDIV
    assert _having(rows, "instGeneral") == INST_GENERAL
    assert _having(rows, "primsInPrims") == PRIMS_IN_PRIMS


def test_every_launch_decision_is_the_one_the_predicates_made(rtc):
    """pool form, pool pays, service kernel, level-free, root cull pre-pass, octet-only sizing and the octLeaf default of the kinds 1..47.
    ACCEL_NONE is launched nowhere (Accel::traceable): its row says no to everything."""
    rows = _rows(rtc)
    assert _having(rows, "pool") == POOL
    assert _having(rows, "poolPays") == POOL_PAYS and POOL_PAYS <= POOL
    assert _having(rows, "service") == SERVICE
    assert _having(rows, "levelFree") == LEVEL_FREE and LEVEL_FREE <= SERVICE
    assert _having(rows, "cull") == CULL == set(range(1, 14))
    assert _having(rows, "octOnly", rtc.KIND_OCT.index("always")) == OCT_ALWAYS
    assert _having(rows, "octOnly", rtc.KIND_OCT.index("quad_form")) == OCT_QUAD_FORM
    assert _having(rows, "octLeaf", 24) == OCT_LEAF_24 and _having(rows, "octLeaf", 16) == set(KINDS) - OCT_LEAF_24
    # the node test launch_cull derived from the kind, for every kind the pre-pass can run on
    assert {k for k in CULL if not rows[k]["robust"]} == CULL_FAST
    assert not any(rows[0][f] for f in ("launcher", "pool", "poolPays", "service", "levelFree", "cull", "octOnly", "primsInPrims"))


def test_a_value_outside_the_enum_is_refused(rtc):
    assert rtc.accel_kind_row(48) is None and rtc.lib().rtcamdDebugAccelKindRow(48) == 0xFFFFFFFF
    assert rtc.accel_kind_row(0xFFFFFFFF) is None and rtc.accel_kind_row(47) is not None


def test_the_bindings_kind_constants_are_distinct_kinds(rtc):
    """every ACCEL_* constant of rtc.py (ACCEL_DATA_* select an array of rtcamdGetAccelData, not a kind) names a kind of its own"""
    consts = {n: getattr(rtc, n) for n in dir(rtc) if n.startswith("ACCEL_") and not n.startswith("ACCEL_DATA_")}
    assert consts and len(set(consts.values())) == len(consts)
    for name, k in consts.items():
        assert rtc.accel_kind_row(k) is not None, name
