"""Every kernel of the wide LSTM library (csrc/lg_lstm_wide.hip -> liblegged_lstm_wide.so) is compared with float64 by at least one GPU
test: a coverage table in the manner of tests/test_lstm_sequence_kernel_coverage.py.  csrc/kernel_resources_lstm_wide.txt (written by
__graft_entry__.build()) lists what hipcc compiled for this library; the table below names, for each symbol, the GPU test functions that
dispatch it and compare its results with a reference.  A new kernel or template instantiation fails this test until a test for it is
added to the table.  (CPU only: the module is parsed, not imported.)"""
import ast
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources_lstm_wide.txt")

GPU = "tests/test_gpu_recurrent_wide.py"
CELL = [f"{GPU}::test_one_step_matches_float64", f"{GPU}::test_one_step_with_weights_times_three_matches_float64",
        f"{GPU}::test_roles_of_different_hidden_size_in_one_launch", f"{GPU}::test_the_wide_cell_equals_the_256_unit_cell_bit_for_bit",
        f"{GPU}::test_a_block_diagonal_512_unit_cell_equals_its_two_256_unit_halves_bit_for_bit", f"{GPU}::test_saturated_gates_stay_finite_and_exact",
        f"{GPU}::test_a_reset_row_ignores_its_stale_state", f"{GPU}::test_24_steps_replay_bit_identically",
        f"{GPU}::test_the_reference_configuration_through_the_wrapper"]
# a pack that misplaces a weight, or that does not run again after the parameters moved, shows in the cell's outputs
CELL_PACK = [f"{GPU}::test_exact_placement_of_every_weight_column", f"{GPU}::test_one_step_matches_float64",
             f"{GPU}::test_load_device_equals_create_and_the_next_launch_sees_new_parameters"]
ACTOR = [f"{GPU}::test_actor_means_match_float64_and_the_flags_do_what_they_say", f"{GPU}::test_the_wide_actor_equals_the_256_unit_actor_bit_for_bit",
         f"{GPU}::test_actor_noise_is_the_reference_stream", f"{GPU}::test_the_reference_configuration_through_the_wrapper"]
ACTOR_PACK = [f"{GPU}::test_actor_means_match_float64_and_the_flags_do_what_they_say", f"{GPU}::test_actor_sync_device_equals_a_fresh_handle"]

COVERAGE = {
    "_ZN2lg16k_lstm_wide_cellENS_12LstmWideArgsE": CELL,
    "_ZN2lg16k_lstm_wide_packEPKfS1_S1_S1_P15HIP_vector_typeIfLj4EES4_iii": CELL_PACK,
    "_ZN2lg17k_lstm_wide_actorENS_13LstmActorArgsE": ACTOR,
    "_ZN2lg22k_lstm_wide_actor_packEPKfS1_PfS2_iii": ACTOR_PACK,
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


def test_every_kernel_of_the_library_has_a_reference_test():
    names = compiled()
    assert len(names) == len(COVERAGE) == 4
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


def test_every_unit_group_shape_is_run():
    """The cell cases hold every wave count of a second group the issue names (288: one wave; 320; 480: seven; 512: eight), odd and even
    K, and the largest LDS block."""
    with open(os.path.join(REPO, GPU)) as f:
        tree = ast.parse(f.read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and any(getattr(x, "id", None) == "CELL_CASES" for x in n.targets))
    assert {h for _, h, _ in cases} == {288, 320, 480, 512} and {i for i, _, _ in cases} == {1, 3, 48, 235, 256}
    assert {n for _, _, n in cases} == {1, 31, 32, 33, 65} and (256, 512) in {(i, h) for i, h, _ in cases}
    assert {(i + h) & 1 for i, h, _ in cases} == {0, 1}


def test_a_new_kernel_is_reported_uncovered(tmp_path):
    extra = ["_ZN2lg16k_lstm_wide_cellILi16EEEvNS_12LstmWideArgsE", "_ZN2lg15k_lstm_wide_gruENS_11GruWideArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources_lstm_wide.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 128  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 2\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
