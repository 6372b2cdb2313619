"""Every compiled kernel that the three other tables (tests/test_kernel_parity_coverage.py, test_learner_kernel_coverage.py,
test_actor_kernel_coverage.py) do not name -- the simulator's small kernels, the game pre / post / outcome kernels and the tail of a PPO
iteration (GAE, gradient clip + Adam, rollout bookkeeping) -- is compared with a reference computed outside the kernel by at least one GPU
test, and the four tables together name every kernel of csrc/kernel_resources.txt exactly once.  The table below names, for each
instantiation, GPU test functions that launch it and compare what it writes with the CPU oracle, a NumPy twin, a recorded step of the
reference or a float64 restatement; a test that only compares two paths of the library with each other is not named.  A new kernel or
instantiation fails this test until a test for it is added to one of the tables.  (CPU only: the modules are parsed, not imported.)

Which call reaches which instantiation (lg_reset_idx, csrc/lg_kernels.hip): k_reset<AnymalTraits, true> for a quadruped driven by the
actuator net (anymal_c_flat, anymal_c_rough, anymal_b), <AnymalTraits, false> for one under PD control (a1), <CassieTraits, false> for the
biped; k_extras follows every one of them.  lg_outcome_post launches k_outcome_post<false>, lg_outcome_pursuer_post k_outcome_post<true>."""
import ast
import os
import re

from tests import test_actor_kernel_coverage as actor_table
from tests import test_kernel_parity_coverage as parity_table
from tests import test_learner_kernel_coverage as learner_table

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")

KERNELS = ("k_obs", "k_reset", "k_extras", "k_actuator", "k_resample_reset",
           "k_game_pre", "k_game_post", "k_dec_pre", "k_dec_post", "k_pursuer_post", "k_outcome_post", "k_dec_outcome", "k_member_outcome",
           "k_gae", "k_adam_sumsq", "k_adam_prepare", "k_adam_update", "k_rollout_record", "k_rollout_post", "k_zero2")

PARITY, SURFACE, TAIL = "tests/test_gpu_parity.py", "tests/test_gpu_env_surface.py", "tests/test_gpu_ppo_tail.py"
GAME, PURSUER, OUTCOME = "tests/test_gpu_game.py", "tests/test_gpu_pursuer_game.py", "tests/test_gpu_outcome.py"
DEC, DEC_OUTCOME, MEMBER = "tests/test_gpu_dec_game.py", "tests/test_gpu_dec_outcome.py", "tests/test_gpu_dec_member_outcome.py"
OBS = f"{PARITY}::test_observations_only_parity"                           # lg_compute_observations_only against the oracle: both builds
# lg_reset_idx against the oracle: anymal_c_flat, cassie, a1, anymal_b; for the two net tasks the subset reset starts from a non-zero actuator
# LSTM state, which only the <AnymalTraits, true> build zeroes (reset envs exactly zero, both layers; the others as loaded)
RESET_ORACLE = f"{PARITY}::test_reset_is_bit_exact"
RESET_RECORDED = f"{PARITY}::test_reset_idx_matches_reference_fixture"     # ... against the reference's recorded reset_idx, episode means included
GAME_RECORDED = f"{GAME}::test_kernels_reproduce_the_recorded_reference_step"          # lg_game_pre + lg_game_post against game_step.npz
GAME_TWIN = f"{GAME}::test_kernels_match_the_twin_on_ragged_sizes"
DEC_RECORDED = f"{DEC}::test_kernels_reproduce_the_recorded_reference_step"
DEC_TWIN = f"{DEC}::test_kernels_match_the_twin_on_ragged_sizes"
OUTCOME_TWIN = f"{OUTCOME}::test_outcome_kernels_match_the_twin_directly"              # per-env arrays of both builds against the twin
OUTCOME_COUNTS = f"{OUTCOME}::test_same_step_bit_for_bit_and_exact_counts"             # counts and means of both builds against the twin
ADAM = [f"{TAIL}::test_adam_kernels_match_float64_on_one_step", f"{TAIL}::test_adam_200_calls_match_200_float64_steps"]
FINISH = f"{TAIL}::test_rollout_finish_kernel_matches_float64"


def reset(traits, net):
    """Mangled name of k_reset<Traits, NET>(KArgs)."""
    return f"_Z7k_resetI{len(traits)}{traits}Lb{int(net)}EEv5KArgs"


def outcome_post(scripted):
    """Mangled name of lg::k_outcome_post<SCRIPTED>(lg_game_params, lg_pursuer_params, lg_game_buffers, lg_outcome_buffers, float *, long)."""
    return f"_ZN2lg14k_outcome_postILb{int(scripted)}EEEv14lg_game_params17lg_pursuer_params15lg_game_buffers18lg_outcome_buffersPfl"


COVERAGE = {
    # the simulator's small kernels
    "_Z5k_obsI12AnymalTraitsEv5KArgs": [OBS],
    "_Z5k_obsI12CassieTraitsEv5KArgs": [OBS],
    reset("AnymalTraits", True): [RESET_ORACLE, RESET_RECORDED],          # (the recorded reset_idx does not read the actuator state: RESET_ORACLE does)
    reset("AnymalTraits", False): [RESET_ORACLE],
    reset("CassieTraits", False): [RESET_ORACLE, RESET_RECORDED],
    "_Z8k_extras5KArgs": [RESET_RECORDED],                                 # extras["episode"] of the reset envs against the recorded means
    "_Z10k_actuatorPKfS0_S0_PfS1_S1_i": [f"{PARITY}::test_actuator_kernel_matches_golden_and_oracle"],
    # the re-draw of the reset envs' commands after a curriculum tick, against the NumPy Philox stream
    "_Z16k_resample_reset5KArgs": [f"{SURFACE}::test_command_curriculum_tick_resamples_the_reset_envs_from_the_widened_range"],
    # the game kernels: recorded reference steps and the NumPy twins
    "_ZN2lg10k_game_preE14lg_game_params15lg_game_buffers": [GAME_RECORDED, GAME_TWIN],
    "_ZN2lg11k_game_postE14lg_game_params15lg_game_buffersl": [GAME_RECORDED, GAME_TWIN, f"{GAME}::test_kernel_reproduces_the_recorded_root_reset"],
    "_ZN2lg9k_dec_preE18lg_dec_game_params19lg_dec_game_buffers": [DEC_RECORDED, DEC_TWIN],
    "_ZN2lg10k_dec_postE18lg_dec_game_params19lg_dec_game_buffersl": [DEC_RECORDED, DEC_TWIN],
    "_ZN2lg14k_pursuer_postE14lg_game_params17lg_pursuer_params15lg_game_buffersPfl": [
        f"{PURSUER}::test_kernel_reproduces_the_recorded_reference_step", f"{PURSUER}::test_kernel_matches_the_twin_on_ragged_sizes",
        f"{PURSUER}::test_speed_limit_is_bit_exact_on_every_episode_step"],
    outcome_post(False): [OUTCOME_TWIN, OUTCOME_COUNTS],
    outcome_post(True): [OUTCOME_TWIN, OUTCOME_COUNTS],
    # as the two k_outcome_post builds: per-env arrays, episode sums and means against the twin itself; counts and rates against the twin
    "_ZN2lg13k_dec_outcomeE18lg_dec_game_params19lg_dec_game_buffers22lg_dec_outcome_buffersl": [
        f"{DEC_OUTCOME}::test_outcome_kernel_matches_the_twin_directly", f"{DEC_OUTCOME}::test_same_step_bit_for_bit_and_exact_counts"],
    "_ZN2lg16k_member_outcomeE18lg_dec_game_params19lg_dec_game_buffers22lg_dec_outcome_buffers29lg_dec_member_outcome_buffersl": [
        f"{MEMBER}::test_member_kernel_matches_the_twin_directly", f"{MEMBER}::test_one_launch_is_bit_identical_to_the_pooled_one_and_counts_per_member_exactly"],
    # the tail of a PPO iteration: float64 restatements (tests/ppo_tail_ref.py)
    "k_gae": [f"{TAIL}::test_gae_kernel_matches_float64", f"{TAIL}::test_gae_through_the_storage"],
    "_ZN2lg12k_adam_sumsqENS_8AdamArgsEl": ADAM,
    "_ZN2lg14k_adam_prepareENS_8AdamArgsE": ADAM,
    "_ZN2lg13k_adam_updateENS_8AdamArgsE": ADAM,
    "_ZN2lg16k_rollout_recordENS_10RecordArgsE": [f"{TAIL}::test_rollout_record_kernel_matches_float64", FINISH],
    "_ZN2lg14k_rollout_postENS_12RollPostArgsE": [FINISH],
    # lg_ppo_loss zeroes stats / d_std with it before k_ppo_loss accumulates: the test hands both NaN-filled
    "k_zero2": ["tests/test_gpu_wide_learner.py::test_ppo_loss_kernel_matches_float64_at_the_games_action_counts"],
}


def kernel_of(symbol):
    """Function name of a symbol in kernel_resources.txt: lg::<name>[<...>] (Itanium: _ZN2lg<len><name>...), a function outside a
    namespace (_Z<len><name>...) or an unmangled name."""
    m = re.match(r"_ZN2lg(\d+)", symbol) or re.match(r"_Z(\d+)", symbol)
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


def all_compiled(path=RESOURCES):
    """Every symbol of a kernel_resources.txt, in file order (comment lines skipped)."""
    with open(path) as f:
        return [line.split()[0] for line in f if line.strip() and not line.startswith("#")]


def compiled_variants(path=RESOURCES):
    """The kernels of this table listed in a kernel_resources.txt."""
    return {s for s in all_compiled(path) if kernel_of(s) in KERNELS}


def uncovered(path=RESOURCES):
    return sorted(compiled_variants(path) - set(COVERAGE))


def test_every_tail_kernel_instantiation_has_a_reference_test():
    names = compiled_variants()
    assert {kernel_of(n) for n in names} == set(KERNELS), sorted(names)
    assert len(names) == len(COVERAGE) == 24                  # 8 simulator-side, 9 game, 7 of the learner's tail
    assert uncovered() == [], "instantiations no GPU test compares with a reference: " + ", ".join(uncovered())
    assert set(COVERAGE) == names, "table entries for kernels that are no longer compiled: " + ", ".join(sorted(set(COVERAGE) - names))


def test_every_named_test_function_exists():
    defined = {}
    for tests in COVERAGE.values():
        assert tests
        for t in tests:
            path, func = t.split("::")
            if path not in defined:
                with open(os.path.join(REPO, path)) as f:
                    tree = ast.parse(f.read())
                gpu = any(isinstance(n, ast.Assign) and any(getattr(x, "id", None) == "pytestmark" for x in n.targets)
                          and "gpu" in ast.unparse(n.value) for n in tree.body)
                defined[path] = ({n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}, gpu)
            funcs, gpu = defined[path]
            assert func in funcs, t
            assert gpu, f"{path} is not marked gpu"


def test_a_new_instantiation_is_reported_uncovered(tmp_path):
    extra = [reset("CassieTraits", True), "_Z5k_obsI8A1TraitsEv5KArgs", "_ZN2lg14k_outcome_postILi2EEEv14lg_game_params17lg_pursuer_params15lg_game_buffers18lg_outcome_buffersPfl",
             "_ZN2lg13k_adam_updateILb1EEEvNS_8AdamArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 256  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 1\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []


def test_the_four_tables_name_every_compiled_kernel_exactly_once(tmp_path):
    tables = {"parity": parity_table.COVERAGE, "learner": learner_table.COVERAGE, "actor": actor_table.COVERAGE, "tail": COVERAGE}
    compiled = all_compiled()
    assert len(compiled) == len(set(compiled)) == 91
    named = [s for t in tables.values() for s in t]
    twice = sorted({s for s in named if named.count(s) > 1})
    assert twice == [], "kernels named by two tables: " + ", ".join(twice)
    assert sorted(named) == sorted(compiled), ("in no table: " + ", ".join(sorted(set(compiled) - set(named)))
                                               + "; no longer compiled: " + ", ".join(sorted(set(named) - set(compiled))))
    # a kernel of a new name belongs to no table's KERNELS: it is reported here
    copy = tmp_path / "kernel_resources.txt"
    with open(RESOURCES) as f:
        copy.write_text(f.read() + "_ZN2lg9k_new_oneENS_7NewArgsE  VGPRs 8  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 8\n")
    assert sorted(set(all_compiled(str(copy))) - set(named)) == ["_ZN2lg9k_new_oneENS_7NewArgsE"]
