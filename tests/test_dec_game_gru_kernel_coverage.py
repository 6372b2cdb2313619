"""The kernel of the shared GRU cell launch (csrc/lg_dec_gru.hip -> liblegged_dec_game_gru.so) is compared with a reference by at least one
GPU test: a coverage table in the manner of tests/test_gru_kernel_coverage.py.  csrc/dec_game_gru_kernel_resources.txt (written by
__graft_entry__.build()) lists what hipcc compiled for this library; the table below names, for each symbol, the GPU test functions that
dispatch it and compare its results with ``lg_gru_step`` and with float64.  A new kernel or template instantiation fails this test until a
test for it is added to the table.  (CPU only: the module is parsed, not imported.)"""
import ast
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "dec_game_gru_kernel_resources.txt")

GPU = "tests/test_gpu_dec_game_gru.py"
CELL = [f"{GPU}::test_four_roles_in_one_launch_equal_each_role_alone_and_float64", f"{GPU}::test_every_pattern_of_present_roles",
        f"{GPU}::test_largest_staged_block_next_to_the_smallest_role", f"{GPU}::test_two_envs_side_by_side_shared_against_separate_launches",
        f"{GPU}::test_graphed_policy_step_equals_the_eager_separate_launches"]

COVERAGE = {
    "_ZN2lg14k_dec_gru_cellENS_10DecGruArgsE": CELL,
}


def compiled(path=RESOURCES):
    names = set()
    with open(path) as f:
        for line in f:
            m = re.match(r"(\S+)\s", line)
            if m and not line.startswith("#"):
                names.add(m.group(1))
    return names


def uncovered(path=RESOURCES):
    return sorted(compiled(path) - set(COVERAGE))


def test_the_one_kernel_of_the_library_has_a_reference_test():
    names = compiled()
    assert len(names) == len(COVERAGE) == 1
    assert uncovered() == [], "kernels no GPU test compares with a reference: " + ", ".join(uncovered())
    assert set(COVERAGE) == names, "table entries for kernels that are no longer compiled: " + ", ".join(sorted(set(COVERAGE) - names))


def test_every_named_test_function_exists_in_a_gpu_module():
    with open(os.path.join(REPO, GPU)) as f:
        tree = ast.parse(f.read())
    assert any(isinstance(n, ast.Assign) and any(getattr(x, "id", None) == "pytestmark" for x in n.targets) and "gpu" in ast.unparse(n.value)
               for n in tree.body), f"{GPU} is not marked gpu"
    funcs = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for tests in COVERAGE.values():
        assert tests
        for t in tests:
            path, func = t.split("::")
            assert path == GPU and func in funcs, t


def test_a_new_kernel_is_reported_uncovered(tmp_path):
    extra = ["_ZN2lg14k_dec_gru_cellILi16EEEvNS_10DecGruArgsE", "_ZN2lg19k_dec_pool_gru_cellENS_14DecPoolGruArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "dec_game_gru_kernel_resources.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 128  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 2\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
