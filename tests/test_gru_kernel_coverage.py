"""Every kernel of the GRU library (csrc/lg_gru.hip -> liblegged_gru.so) is compared with float64 by at least one GPU test: a coverage table
in the manner of tests/test_lstm_wide_kernel_coverage.py.  csrc/kernel_resources_gru.txt (written by __graft_entry__.build()) lists what
hipcc compiled for this library; the table below names, for each symbol, the GPU test functions that dispatch it and compare its results
with a reference.  A new kernel or template instantiation fails this test until a test for it is added to the table.  (CPU only: the
module is parsed, not imported.)"""
import ast
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources_gru.txt")

GPU = "tests/test_gpu_recurrent_gru.py"
CELL = [f"{GPU}::test_one_step_matches_float64", f"{GPU}::test_one_step_with_weights_times_three_matches_float64",
        f"{GPU}::test_roles_of_different_hidden_size_in_one_launch", f"{GPU}::test_a_saturated_update_gate_returns_h_in_bit_for_bit",
        f"{GPU}::test_closed_gates_return_the_candidate_of_x_alone", f"{GPU}::test_pre_activations_at_1e4_stay_finite",
        f"{GPU}::test_a_reset_row_ignores_its_stale_state", f"{GPU}::test_24_steps_with_resets_match_float64_and_replay_bit_identically",
        f"{GPU}::test_recurrent_fused_actor_follows_the_module_and_draws_the_fused_actors_noise"]
# a pack that misplaces a weight, or that does not run again after the parameters moved, shows in the cell's outputs
PACK = [f"{GPU}::test_exact_placement_of_every_weight_column", f"{GPU}::test_one_step_matches_float64",
        f"{GPU}::test_closed_gates_return_the_candidate_of_x_alone", f"{GPU}::test_load_device_equals_create_and_the_next_launch_sees_new_parameters"]

COVERAGE = {
    "_ZN2lg10k_gru_cellENS_7GruArgsE": CELL,
    "_ZN2lg10k_gru_packEPKfS1_S1_S1_P15HIP_vector_typeIfLj4EES4_iii": PACK,
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


def test_a_new_kernel_is_reported_uncovered(tmp_path):
    extra = ["_ZN2lg10k_gru_cellILi16EEEvNS_7GruArgsE", "_ZN2lg14k_gru_sequenceENS_10GruSeqArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources_gru.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 128  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 2\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
