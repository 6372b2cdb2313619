"""Every kernel of liblegged_dec_game_recurrent.so (csrc/lg_dec_game_lstm_act.hip) is compared with a reference computed outside the kernel
by at least one GPU test, in the manner of tests/test_actor_kernel_coverage.py: csrc/kernel_resources_dec_game_recurrent.txt (written by
__graft_entry__.build()) lists what hipcc compiled, the table below names the GPU tests that launch each kernel and compare its results
with the stand-alone launches, float64 or the Philox reference.  A further instantiation fails this test until a test for it is added to
the table.  (CPU only: the modules are parsed, not imported.)"""
import ast
import os

from tests.test_actor_kernel_coverage import kernel_of

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources_dec_game_recurrent.txt")
KERNELS = ("k_dec_lstm_cell", "k_dec_game_lstm_act")
GPU = "tests/test_gpu_dec_game_recurrent.py"

COVERAGE = {
    # the cell launch: every role set against lg_lstm_step with the role alone (bits), all four roles against float64
    "_ZN2lg15k_dec_lstm_cellENS_11DecLstmArgsE": [f"{GPU}::test_cell_launch_is_bit_identical_to_each_role_alone", f"{GPU}::test_cell_launch_matches_float64"],
    # the actor launch: against the separate launches (bits), the NumPy twin of the clips, float64 forwards and log-probs, the Philox reference
    "_ZN2lg19k_dec_game_lstm_actENS_18DecGameLstmActArgsE": [f"{GPU}::test_actor_launch_is_bit_identical_to_the_separate_launches",
                                                           f"{GPU}::test_clip_and_wrap_are_exercised_on_both_sides",
                                                           f"{GPU}::test_actor_launch_matches_float64_forwards_and_log_probs",
                                                           f"{GPU}::test_noise_is_the_reference_philox_stream_under_each_agents_seed"],
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
    extra = ["_ZN2lg15k_dec_lstm_cellILi2EEEvNS_11DecLstmArgsE", "_ZN2lg19k_dec_game_lstm_actILb1EEEvNS_18DecGameLstmActArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources_dec_game_recurrent.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 256  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 1\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
