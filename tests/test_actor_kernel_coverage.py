"""Every compiled instantiation of the rollout-path policy kernels -- the stand-alone actors (csrc/lg_policy.h), the shared actor launches
of the game tasks (csrc/lg_game_act.h, lg_dec_game.hip, lg_pool_act.hip), the recurrent cell and its actor (csrc/lg_recurrent.hip) and
their weight-packing kernels -- is compared with a reference computed outside the kernel by at least one GPU test.
csrc/kernel_resources.txt (written by __graft_entry__.build()) lists what hipcc compiled; the table below names, for each instantiation,
the GPU test functions that dispatch it and compare its results with a float64 restatement or the torch forward.  A new template
instantiation fails this test until a test for it is added to the table.  (CPU only: the modules are parsed, not imported.)

Which call reaches which instantiation (lg_policy_act in csrc/lg_learner.hip): TILES0 = ceil(observations / 16).  The 48-128-64-32 actor
always runs k_policy_act<3, 8, 4, 2>.  A 512-256-128 actor runs k_policy_act_wide<TILES0, 16, 8, 4> at lg_mlp_wide_set_precision(1), the
default, and k_policy_act<TILES0, 32, 16, 8> at precision 0; the tests named for them are parametrised over both settings.  The tests of
tests/test_gpu_actor_edges.py take every one of the nine to the first and last observation width of its range, to env counts on every
side of a workgroup and to 1 .. 16 actions against float64 (tests/actor_check.py holds the table and restates this dispatch)."""
import ast
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")

KERNELS = ("k_policy_act", "k_policy_act_wide", "k_prey_act", "k_dec_act", "k_pool_act", "k_policy_pack", "k_policy_pack_wide",
           "k_lstm_cell", "k_lstm_pack", "k_lstm_actor", "k_lstm_actor_pack")

SURFACE, GAME, DEC, POOL = "tests/test_gpu_env_surface.py", "tests/test_gpu_game_policy.py", "tests/test_gpu_dec_game.py", "tests/test_gpu_dec_pool.py"
ORACLE, CELL, ACTOR = "tests/test_gpu_rollout_oracle.py", "tests/test_gpu_recurrent.py", "tests/test_gpu_recurrent_actor.py"
TORCH = f"{SURFACE}::test_fused_actor_matches_torch_forward"               # 48 / 235 / 169 observations against the torch forward, both precisions
NOISE = f"{ORACLE}::test_policy_act_noise_matches_the_reference"           # the same three shapes: actions - mean against the Philox reference
REPACK = f"{SURFACE}::test_fused_actor_follows_the_optimiser_through_the_device_repack"      # sync_device(), then the torch forward: 48 and 235
GAME_SHAPE = f"{GAME}::test_game_actor_shape_matches_torch_forward"        # 19 observations, both precisions, sync_device() in both
ONE_TILE = f"{DEC}::test_one_tile_actor_shapes_match_torch_forward"        # 16 and 3 observations, both precisions, sync_device() in both
CELL_STEP = f"{CELL}::test_one_step_matches_float64"
CELL_TESTS = [CELL_STEP, f"{CELL}::test_roles_of_different_hidden_size_in_one_launch", f"{CELL}::test_exact_placement_of_every_weight_column",
              f"{CELL}::test_24_steps_with_resets_match_float64_and_replay_bit_identically", f"{CELL}::test_saturated_gates_stay_finite_and_exact",
              f"{CELL}::test_a_reset_row_ignores_its_stale_state"]
ACTOR_MEANS = f"{ACTOR}::test_means_match_float64_and_the_flags_do_what_they_say"
ACTOR_NOISE = f"{ACTOR}::test_noise_is_the_reference_stream_for_every_action_count_and_step_source"
ACTOR_SYNC = f"{ACTOR}::test_sync_device_equals_a_fresh_handle"
ROUGH_DEFAULT = f"{CELL}::test_default_policy_of_the_rough_task_through_the_wrapper"
EDGES = "tests/test_gpu_actor_edges.py"                                    # tests/actor_check.py: every kernel at its width, env-count and action-count edges
EDGE_MEANS = f"{EDGES}::test_means_match_float64_with_guard_rows_intact"   # float64, NaN guard rows; host pack, then lg_policy_load_device bit-equal
EDGE_FLAGS = f"{EDGES}::test_flags_at_a_ragged_case"
EDGE_NOISE = f"{EDGES}::test_noise_is_the_reference_stream_for_every_action_count"      # 19 observations, 1 .. 16 actions, both precisions
EDGE_REPACK = f"{EDGES}::test_device_repack_equals_host_pack_at_the_padded_widths"      # sync_device() at each range's first and last width
EDGE = [EDGE_MEANS, EDGE_FLAGS, EDGE_REPACK]


def policy_act(t0, t1, t2, t3):
    """Mangled name of lg::k_policy_act<T0, T1, T2, T3>(lg::PolicyArgs)."""
    return f"_ZN2lg12k_policy_actILi{t0}ELi{t1}ELi{t2}ELi{t3}EEEvNS_10PolicyArgsE"


def policy_act_wide(t0):
    """Mangled name of lg::k_policy_act_wide<T0, 16, 8, 4>(lg::PolicyWideArgs)."""
    return f"_ZN2lg17k_policy_act_wideILi{t0}ELi16ELi8ELi4EEEvNS_14PolicyWideArgsE"


COVERAGE = {
    # exact-f32 actors: the flat shape at either precision, the 512-256-128 shapes at precision 0
    policy_act(3, 8, 4, 2): [TORCH, NOISE, REPACK] + EDGE,
    policy_act(15, 32, 16, 8): [TORCH, NOISE] + EDGE,                      # rough: 235 observations
    policy_act(11, 32, 16, 8): [TORCH, NOISE] + EDGE,                      # cassie: 169
    policy_act(2, 32, 16, 8): [GAME_SHAPE, EDGE_NOISE] + EDGE,            # high_level_game: 19
    policy_act(1, 32, 16, 8): [ONE_TILE] + EDGE,                          # dec_high_level_game: 16 and 3
    # split-bf16 actors: the same shapes at precision 1
    policy_act_wide(15): [TORCH, NOISE, REPACK] + EDGE,
    policy_act_wide(11): [TORCH, NOISE] + EDGE,
    policy_act_wide(2): [GAME_SHAPE, EDGE_NOISE] + EDGE,
    policy_act_wide(1): [ONE_TILE] + EDGE,
    # the shared actor launches of the game tasks: float64 forwards of every role at n = 33
    "_ZN2lg10k_prey_actENS_11PreyActArgsE": [f"{GAME}::test_shared_actor_launch_matches_float64_forwards"],
    "_ZN2lg9k_dec_actENS_10DecActArgsE": [f"{DEC}::test_shared_actor_launch_matches_float64_forwards"],
    "_ZN2lg10k_pool_actENS_11PoolActArgsE": [f"{POOL}::test_pooled_launch_matches_float64_forwards_of_each_blocks_member"],
    # weight packing on the device (sync_device()): the f32 layout is read by the precision-0 kernels and the flat actor, the split-bf16
    # layout by the precision-1 kernels, whose handles pack it at creation too
    "_Z13k_policy_packPKfS0_iiiiPfS1_": [REPACK, GAME_SHAPE, ONE_TILE, EDGE_MEANS, EDGE_REPACK],
    "_ZN2lg18k_policy_pack_wideEPKfS1_iiiiiPDF16bPf": [TORCH, REPACK, GAME_SHAPE, ONE_TILE, EDGE_MEANS, EDGE_REPACK],
    # the recurrent policy: the cell (lg_lstm_create packs on the device) and the actor behind it (every handle packs on the device)
    "_ZN2lg11k_lstm_cellENS_8LstmArgsE": CELL_TESTS + [ROUGH_DEFAULT],
    "_ZN2lg11k_lstm_packEPKfS1_S1_S1_P15HIP_vector_typeIfLj4EES4_iii": [CELL_STEP, f"{CELL}::test_load_device_equals_create"],
    "_ZN2lg12k_lstm_actorENS_13LstmActorArgsE": [ACTOR_MEANS, ACTOR_NOISE, ACTOR_SYNC, ROUGH_DEFAULT],
    "_ZN2lg17k_lstm_actor_packEPKfS1_PfS2_iii": [ACTOR_MEANS, ACTOR_SYNC],
}


def kernel_of(symbol):
    """Function name of a symbol in kernel_resources.txt: lg::<name>[<...>] (Itanium: _ZN2lg<len><name>...), a function outside a
    namespace (_Z<len><name>...) or an unmangled name."""
    m = re.match(r"_ZN2lg(\d+)", symbol) or re.match(r"_Z(\d+)", symbol)
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


def compiled_variants(path=RESOURCES):
    """The rollout-path policy kernels listed in a kernel_resources.txt."""
    names = set()
    with open(path) as f:
        for line in f:
            m = re.match(r"(\S+)\s", line)
            if m and not line.startswith("#") and kernel_of(m.group(1)) in KERNELS:
                names.add(m.group(1))
    return names


def uncovered(path=RESOURCES):
    return sorted(compiled_variants(path) - set(COVERAGE))


def test_every_actor_kernel_instantiation_has_a_reference_test():
    names = compiled_variants()
    assert {kernel_of(n) for n in names} == set(KERNELS), sorted(names)
    assert len(names) == len(COVERAGE) == 18                  # 5 + 4 actors, 3 shared launches, 2 pack kernels; the cell, the recurrent actor, their 2 pack kernels
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
    extra = [policy_act(4, 32, 16, 8), policy_act_wide(4), "_ZN2lg12k_lstm_actorILi8EEEvNS_13LstmActorArgsE", "_ZN2lg10k_pool_actILb1EEEvNS_11PoolActArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 256  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 1\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
