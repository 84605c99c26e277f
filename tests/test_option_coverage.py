"""Every tuning knob of the library (g_fx_options in csrc/fistr_hip.hip) is either run by the variant tests against the oracle
(tests/test_gpu_kernel_variants.py) or exempted here with its reason: a knob added without a test or a reason fails the CPU suite."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXEMPT = {
    "FX_ARENA_GB": "value arena: test_arena_walk_keeps_the_answers_bit_identical, test_value_arena_places_reuses_and_falls_back",
    "FX_ARENA_GOOD_GBS": "value arena verification: test_arena_walk_keeps_the_answers_bit_identical",
    "FX_ARENA_TRIES": "value arena verification: test_arena_walk_keeps_the_answers_bit_identical",
    "FX_ARENA_MAX_MB": "value arena cap: test_value_arena_places_reuses_and_falls_back",
    "FX_ARENA_THRESHOLD_MB": "value arena threshold: test_arena_walk_keeps_the_answers_bit_identical",
    "FX_BFS_DEVICE_MIN": "device level ordering: test_device_level_ordering_*, test_gpu_nn_shapes.py::test_device_ordering_equals_host_ordering",
    "FX_BFS_BATCH": "device level ordering: test_device_level_ordering_disconnected_graph_takes_host_walk",
    "FX_MC_DEVICE_MIN": "device multicolouring: test_device_level_ordering_*, test_gpu_nn_shapes.py::test_device_ordering_equals_host_ordering",
    "FX_MC_BATCH": "device multicolouring: test_device_level_ordering_equals_host_ordering",
    "FX_VAL2_POW2": "allocation size of value arrays of 1 GiB or more outside the arena: placement only, no kernel or data change",
    "FX_GRAPH": "graph capture of the Krylov loop: test_graph_replay_is_bit_identical",
    "FX_OVERLAP": "halo exchange overlap of decomposed systems: test_gpu_distributed",
    "FX_DF_GRID": "dataflow grid clamp: test_dataflow_grid_is_clamped_to_the_co_resident_bound, test_dataflow_sweeps_equal_launch_per_level_sweeps_bitwise, test_gpu_nn_shapes.py::test_ilu_sweep_forms_bitwise",
    "FX_MARCH": "plane march: test_march_*",
    "FX_MARCH_CHUNK": "plane march: test_march_*",
    "FX_MARCH_WAVES": "plane march: test_march_*",
    "FX_MARCH_GRID": "plane march: test_march_*",
    "FX_MARCH_XCD": "plane march: test_march_*",
    "FX_DEBUG_DF_FAIL": "test hook of the dataflow fallback: test_timed_out_dataflow_sweep_falls_back_to_level_sweeps",
    "FX_DEBUG_ONECOLOR": "measurement only: ignores the colour dependencies, wrong numbers by design",
}


def library_options():
    src = open(os.path.join(ROOT, "frontistr_amd", "csrc", "fistr_hip.hip")).read()
    table = src[src.index("g_fx_options[] = {"):]
    table = table[:table.index("\n};")]
    return re.findall(r'\{"(FX_[A-Z0-9_]+)"', table)


def variant_table():
    """The option names the variant tests set (parsed, not imported: that module needs a GPU)."""
    src = open(os.path.join(ROOT, "tests", "test_gpu_kernel_variants.py")).read()
    body = src[src.index("VARIANT_ENV = ("):]
    body = body[:body.index(")\n")]
    live = src[src.index("LIVE_OPTIONS = ["):]
    live = live[:live.index("\n]")]
    return set(re.findall(r'"(FX_[A-Z0-9_]+)"', body)), set(re.findall(r'\("(FX_[A-Z0-9_]+)"', live))


def test_every_option_is_tested_or_exempted():
    names = library_options()
    assert len(names) >= 40 and len(set(names)) == len(names)
    variants, live = variant_table()
    missing = [n for n in names if n not in variants and n not in EXEMPT]
    assert not missing, "FX_* options with neither a variant test nor an exemption: %s" % missing
    assert not (variants & set(EXEMPT)), "both tested and exempted: %s" % sorted(variants & set(EXEMPT))
    stale = sorted((variants | set(EXEMPT)) - set(names))
    assert not stale, "names that are no option of the library: %s" % stale
    assert live <= variants, sorted(live - variants)
    # every option of the variant table is also flipped on a live context
    assert variants - live == set(), sorted(variants - live)


# FX_* environment variables the library reads itself (getenv under csrc/) that are not tuning knobs of g_fx_options: the test
# that runs each of them, or why none does
ENV_ONLY = {
    "FX_ASM_ATOMIC": "atomic stiffness scatter: test_gpu_assembly_meshes.py (atomic, atomic_map0 children), "
                     "test_assembly_coloured_scatter_is_reproducible_and_equals_atomic_scatter",
    "FX_ASM_MAP": "binary-search scatter: test_gpu_assembly_meshes.py (map0, atomic_map0 children)",
    "FX_ASM_FIRST": "read-modify-write scatter after clearing: test_gpu_assembly_meshes.py (first0 child)",
    "FX_TIMING": "prints host phase timings to stderr: diagnostics only, no kernel or data change",
    "FX_HOST_THREADS": "host thread count of the orderings and the profile build: same results for any count, no kernel change",
    "FX_HALO_COMM": "0: halo exchange on the all-reduce communicator instead of a split one (ordering only, same data); "
                    "the split communicator of multi-rank runs is the tested default (test_gpu_distributed)",
    "FX_FORCE_COMM": "in-stream communicator on one rank: test_gpu_distributed (FX_FORCE_COMM=1 child)",
    "FX_DEBUG_ARENA_GB": "size of the placement arena of the debug allocator (fx_debug_host.h): measurement tooling, not the product path",
    "FX_MARCH_CHECK": "host self-check of every plane march program (always on for small systems, so test_march_* run it): "
                      "verification only, no result change",
}


def library_getenv_names():
    names = set()
    d = os.path.join(ROOT, "frontistr_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip", ".cpp", ".c")):
            names |= set(re.findall(r'getenv\("(FX_[A-Z0-9_]+)"\)', open(os.path.join(d, f)).read()))
    return names


def test_every_environment_switch_is_tested_or_exempted():
    names = library_getenv_names()
    options = set(library_options())
    env_only = names - options
    missing = sorted(env_only - set(ENV_ONLY))
    assert not missing, "FX_* environment variables read outside g_fx_options with neither a test nor a reason: %s" % missing
    stale = sorted(set(ENV_ONLY) - env_only)
    assert not stale, "listed but not read by the library (or now an option of g_fx_options): %s" % stale
    assert all(ENV_ONLY[n].strip() for n in ENV_ONLY)
