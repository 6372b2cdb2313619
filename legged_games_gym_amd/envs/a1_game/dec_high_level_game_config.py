"""``DecHighLevelGameCfg / DecHighLevelGameCfgPPO`` (reference ``legged_gym/envs/a1_game/dec_high_level_game_config.py``).

The values are pinned by tests/golden/dec_game_configs.json, the ``class_to_dict`` dump of the reference's own classes
(tools/make_dec_game_golden.py).  One field is new: ``env.ll_policy_path`` (see ``DecHighLevelGame``)."""
from ..base.base_config import BaseConfig


class DecHighLevelGameCfg(BaseConfig):
    class env:
        capture_dist = 0.5            # the prey is captured when the predator is closer than this [m]
        env_spacing = 3.0
        episode_length_s = 20
        num_actions_predator = 2      # predator (lin_vel_x, lin_vel_y)
        num_actions_prey = 4          # prey (lin_vel_x, lin_vel_y, ang_vel_yaw, heading)
        num_envs = 2000
        num_observations_predator = 3     # prey position relative to the predator
        num_observations_prey = 16        # 4 x sensed relative predator position + 4 visibility flags
        num_privileged_obs_predator = None
        num_privileged_obs_prey = None
        send_timeouts = True
        # NEW (not in the reference, which hard-codes a run directory, dec_high_level_game.py:99): checkpoint of the frozen low-level policy;
        # None = the newest checkpoint of the `a1` experiment (get_load_path with the a1 train cfg's load_run / checkpoint)
        ll_policy_path = None

    class terrain:
        curriculum = False
        mesh_type = "plane"
        num_cols = 20
        num_rows = 10

    class commands:
        heading_command = True

        class ranges:
            ang_vel_yaw = [-1, 1]
            heading = [-3.14, 3.14]
            lin_vel_x = [-1.0, 1.0]
            lin_vel_y = [-1.0, 1.0]
            predator_lin_vel_x = [-2.0, 2.0]
            predator_lin_vel_y = [-2.0, 2.0]

    class init_state:
        ang_vel = [0.0, 0.0, 0.0]
        default_joint_angles = {
            "FL_hip_joint": 0.1, "RL_hip_joint": 0.1, "FR_hip_joint": -0.1, "RR_hip_joint": -0.1,
            "FL_thigh_joint": 0.8, "RL_thigh_joint": 1.0, "FR_thigh_joint": 0.8, "RR_thigh_joint": 1.0,
            "FL_calf_joint": -1.5, "RL_calf_joint": -1.5, "FR_calf_joint": -1.5, "RR_calf_joint": -1.5,
        }
        lin_vel = [0.0, 0.0, 0.0]
        pos = [0.0, 0.0, 0.42]
        predator_pos = [0.0, 0.0, 0.3]
        rot = [0.0, 0.0, 0.0, 1.0]

    class domain_rand:
        added_mass_range = [-1.0, 1.0]
        friction_range = [0.5, 1.25]
        max_push_vel_xy = 1.0
        push_interval_s = 15
        push_robots = True
        randomize_base_mass = False
        randomize_friction = True

    class rewards_prey:
        only_positive_rewards = True

        class scales:
            evasion = 0.9

    class rewards_predator:
        only_positive_rewards = False

        class scales:
            pursuit = 0.9

    class noise:
        add_noise = True
        noise_level = 1.0

    class viewer:
        lookat = [11.0, 5, 3.0]
        pos = [10, 0, 6]
        ref_env = 0

    class sim:
        dt = 0.005
        gravity = [0.0, 0.0, -9.81]
        substeps = 1
        up_axis = 1

        class physx:
            bounce_threshold_velocity = 0.5
            contact_collection = 2
            contact_offset = 0.01
            default_buffer_size_multiplier = 5
            max_depenetration_velocity = 1.0
            max_gpu_contact_pairs = 2 ** 23
            num_position_iterations = 4
            num_threads = 10
            num_velocity_iterations = 0
            rest_offset = 0.0
            solver_type = 1


class DecHighLevelGameCfgPPO(BaseConfig):
    runner_class_name = "OnPolicyRunner"
    seed = 1

    class policy:
        activation = "elu"
        actor_hidden_dims = [512, 256, 128]
        critic_hidden_dims = [512, 256, 128]
        init_noise_std = 1.0

    class algorithm:
        clip_param = 0.2
        desired_kl = 0.01
        entropy_coef = 0.01
        gamma = 0.99
        lam = 0.95
        learning_rate = 1.0e-3
        max_grad_norm = 1.0
        num_learning_epochs = 5
        num_mini_batches = 4
        schedule = "adaptive"
        use_clipped_value_loss = True
        value_loss_coef = 1.0

    class runner:
        algorithm_class_name = "PPO"
        checkpoint = -1
        experiment_name = "dec_high_level_game"
        load_run = -1
        max_evolutions = 20           # how often predator and prey alternate; every evolution trains one agent for max_iterations
        max_iterations = 200          # policy updates per evolution
        num_steps_per_env = 24
        policy_class_name = "ActorCritic"
        resume = False
        resume_path = None
        run_name = ""
        save_interval = 50
