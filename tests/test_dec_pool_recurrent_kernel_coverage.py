"""Every kernel of liblegged_dec_pool_recurrent.so (csrc/lg_dec_pool_lstm_act.hip) is compared with a reference computed outside the kernel
by at least one GPU test, in the manner of tests/test_dec_game_recurrent_kernel_coverage.py: csrc/kernel_resources_dec_pool_recurrent.txt
(written by __graft_entry__.build()) lists what hipcc compiled, the table below names the GPU tests that launch each kernel and compare its
results with the plain launches per block or with float64.  A further instantiation fails this test until a test for it is added to the
table.  (CPU only: the modules are parsed, not imported.)"""
import ast
import os

from tests.test_actor_kernel_coverage import kernel_of

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources_dec_pool_recurrent.txt")
KERNELS = ("k_dec_pool_lstm_cell", "k_dec_pool_lstm_act")
GPU = "tests/test_gpu_dec_pool_recurrent.py"

COVERAGE = {
    # the pooled cell launch: per block against lg_dec_lstm_step with the block's member (bits), per block against float64
    "_ZN2lg20k_dec_pool_lstm_cellENS_15DecPoolLstmArgsE": [f"{GPU}::test_pooled_cell_launch_is_bit_identical_per_block_to_the_plain_launch_with_the_blocks_member",
                                                          f"{GPU}::test_pooled_launches_match_float64_per_block_with_the_blocks_member"],
    # the pooled actor launch: per block against lg_dec_game_lstm_act with the block's member (bits), float64 forwards and log-probs per block
    "_ZN2lg19k_dec_pool_lstm_actENS_18DecPoolLstmActArgsE": [f"{GPU}::test_pooled_actor_launch_is_bit_identical_per_block_to_the_plain_launch_with_the_blocks_member",
                                                           f"{GPU}::test_pooled_launches_match_float64_per_block_with_the_blocks_member"],
}


def compiled(path=RESOURCES):
    with open(path) as f:
        return {line.split()[0] for line in f if line.strip() and not line.startswith("#")}


def uncovered(path=RESOURCES):
    return sorted(compiled(path) - set(COVERAGE))


def test_every_kernel_of_the_library_has_a_reference_test():
    names = compiled()
    assert {kernel_of(n) for n in names} == set(KERNELS), sorted(names)
    assert len(names) == len(COVERAGE) == 2
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


def test_a_further_instantiation_is_reported_uncovered(tmp_path):
    extra = ["_ZN2lg20k_dec_pool_lstm_cellILi2EEEvNS_15DecPoolLstmArgsE", "_ZN2lg19k_dec_pool_lstm_actILb1EEEvNS_18DecPoolLstmActArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources_dec_pool_recurrent.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 256  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 1\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
