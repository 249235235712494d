#!/bin/bash
# A/B builds: tools/build_variant.sh NAME "-DFLAG ..."  ->  rogue-gym_amd/variants/librogue_NAME.so (select with ROGUE_GYM_HIP_LIB=...).
# The same translation units and -O levels as csrc/build.sh (units.sh), compiled side by side.  The variant .so files are git-ignored.
set -e
name=$1; shift
cd "$(dirname "$0")/../rogue-gym_amd/csrc"
. ./units.sh
B=../build_$name; mkdir -p $B ../variants
F="--offload-arch=gfx950 -std=c++17 -fPIC -Wall -Wno-unused-function -DRG_BUILD_ID=\"variant-$name\" $*"
OBJS=; PIDS=
for u in $UNITS; do
    src=${u%%:*}; obj=$B/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj &
    PIDS="$PIDS $!"; OBJS="$OBJS $obj"
done
FOBJS=
for u in $OBSFIX_UNITS; do   # the group-wise fix-up pass takes the variant's flags too (-DOBS_FIX_GROUP=..., -DOBS_FIX_AHEAD=...): a library of the variant's own
    src=${u%%:*}; obj=$B/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj &
    PIDS="$PIDS $!"; FOBJS="$FOBJS $obj"
done
EOBJS=
for u in $STEPENC_UNITS; do  # ... and so does the step kernel of the headline class (k_step_enc)
    src=${u%%:*}; obj=$B/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj &
    PIDS="$PIDS $!"; EOBJS="$EOBJS $obj"
done
for p in $PIDS; do wait $p; done   # (a failed compile ends the script: set -e)
hipcc --offload-arch=gfx950 -shared $FOBJS -o ../variants/librogue_gym_obsfix_$name.so
hipcc --offload-arch=gfx950 -shared $EOBJS -o ../variants/librogue_gym_stepenc_$name.so
# (the novelty pass, the cell archive, the policy pass, its learner's side and the returns pass are the product's own libraries beside the variant's directory: csrc/build.sh or __graft_entry__.build() made them)
hipcc --offload-arch=gfx950 -shared $OBJS -L.. -L../variants -lrogue_gym_novelty -lrogue_gym_archive -lrogue_gym_policy -lrogue_gym_learn -lrogue_gym_returns -lrogue_gym_obsfix_$name -lrogue_gym_stepenc_$name '-Wl,-rpath,$ORIGIN/..:$ORIGIN' -o ../variants/librogue_$name.so
echo "built variants/librogue_$name.so"
