# The translation units of librogue_gym_hip.so and the optimisation level of each, in link order: THE list, sourced by build.sh and tools/build_variant.sh and
# read by __graft_entry__.build() (which sources this file in a shell and prints the variables).
# The step kernels want -O3; the bandwidth-bound render/observation kernels are faster with -Os (less unrolling).  The host units (rg_api*.cpp: the C-ABI by
# subsystem, DESIGN.md "The host layer") take -O2.
UNITS="rg_kernels.hip:-O3 rg_regen_lanes.hip:-O3 rg_obs.hip:-Os rg_crop_typed.hip:-Os rg_pixels.hip:-Os rg_action_mask.hip:-Os rg_path.hip:-O3 rg_route.hip:-O3
       rg_episode.hip:-O3 rg_monsters.hip:-O3 rg_objects.hip:-O3 rg_state_io.hip:-O3
       rg_api.cpp:-O2 rg_api_obs.cpp:-O2 rg_api_readers.cpp:-O2 rg_api_learn.cpp:-O2 rg_api_episode.cpp:-O2 rg_api_state.cpp:-O2 rg_api_comm.cpp:-O2 rg_api_diag.cpp:-O2
       rg_config.cpp:-O2 rg_items.cpp:-O2"
# The novelty pass is a library of its own, librogue_gym_novelty.so, which librogue_gym_hip.so links (found beside it at run time): its kernels stay out of the
# code objects whose kernel set tests/test_pixels_resources.py pins by name.
NOVELTY_UNITS="rg_novelty.hip:-O3"
# The cell archive likewise, librogue_gym_archive.so: its record writers are rg_state_save's bodies (rg_state_io_dev.h) under kernel names of their own.
ARCHIVE_UNITS="rg_archive.hip:-O3"
# The group-wise fix-up pass likewise, librogue_gym_obsfix.so: k_obs_fix shares its Redraw service with rg_obs.hip through rg_obs_dev.h (-Os, as that unit).
OBSFIX_UNITS="rg_obs_fix.hip:-Os"
# The step kernel of the headline class likewise, librogue_gym_stepenc.so: k_step_enc is rg_kernels.hip's turn code (which the unit includes) compiled for the
# 32 x 16 grid alone (-O3, as that unit); k_step_w32<false, true> keeps its place and its registers in librogue_gym_hip.so.
STEPENC_UNITS="rg_step_enc.hip:-O3"
# The masked categorical action from policy logits likewise, librogue_gym_policy.so: k_act states rg_policy.h's rule, which the host twin shares (-O3: the rule
# is arithmetic, three short passes over a row).
POLICY_UNITS="rg_policy.hip:-O3"
# The learner's side of that rule likewise, librogue_gym_learn.so: k_pg_eval and k_pg_grad state rg_policy_grad.h's rule (log-probability of stored actions, entropy
# under stored masks, their gradient), which the host twins share; librogue_gym_policy.so stays the three k_act instances (-O3, as that unit).
LEARN_UNITS="rg_policy_grad.hip:-O3"
# Returns and advantages of a [T, N] rollout likewise, librogue_gym_returns.so: k_gae and k_vtrace state rg_returns.h's rule (GAE, reward-to-go, V-trace), which the
# host twins share (-O3: a register pipeline of loads around a short dependent chain).
RETURNS_UNITS="rg_returns.hip:-O3"
# The units of UNITS that the development library (variants/librogue_gym_hip_dev.so) compiles again with -DRG_DEV_KNOBS; it links the product's objects of all others.
# Of the host units only the core reads the environment (tests/test_novelty_resources.py).
KNOB_UNITS="rg_kernels.hip rg_regen_lanes.hip rg_obs.hip rg_api.cpp"
