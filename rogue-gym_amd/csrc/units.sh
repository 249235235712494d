# The translation units of librogue_gym_hip.so and the optimisation level of each, in link order; sourced by build.sh and tools/build_variant.sh.
# The step kernels want -O3; the bandwidth-bound render/observation kernels are faster with -Os (less unrolling).
UNITS="rg_kernels.hip:-O3 rg_regen_lanes.hip:-O3 rg_obs.hip:-Os rg_crop_typed.hip:-Os rg_pixels.hip:-Os rg_action_mask.hip:-Os rg_path.hip:-O3 rg_route.hip:-O3
       rg_episode.hip:-O3 rg_monsters.hip:-O3 rg_objects.hip:-O3 rg_state_io.hip:-O3 rg_api.cpp:-O2 rg_config.cpp:-O2 rg_items.cpp:-O2"
# The novelty pass is a library of its own, librogue_gym_novelty.so, which librogue_gym_hip.so links (found beside it at run time): its kernels stay out of the
# code objects whose kernel set tests/test_pixels_resources.py pins by name.
NOVELTY_UNITS="rg_novelty.hip:-O3"
