#!/bin/bash
# Builds librogue_gym_hip.so, librogue_gym_novelty.so, librogue_gym_archive.so, librogue_gym_obsfix.so, librogue_gym_stepenc.so, librogue_gym_policy.so, librogue_gym_learn.so and librogue_gym_returns.so for gfx950 in-tree (cross-compiles without a GPU).  The translation units and
# their -O levels: units.sh.
set -e
cd "$(dirname "$0")"
. ./units.sh
OUT=../librogue_gym_hip.so
ID=$(python3 -c "import sys; sys.path.insert(0, '../..'); import __graft_entry__ as g; print(g.source_id())")   # compiled in as rg_build_id()
F="--offload-arch=gfx950 -std=c++17 -fPIC -Wall -Wno-unused-function -DRG_BUILD_ID=\"$ID\""
mkdir -p ../build
OBJS=
for u in $UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    OBJS="$OBJS $obj"
done
NOBJS=
for u in $NOVELTY_UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    NOBJS="$NOBJS $obj"
done
AOBJS=
for u in $ARCHIVE_UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    AOBJS="$AOBJS $obj"
done
FOBJS=
for u in $OBSFIX_UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    FOBJS="$FOBJS $obj"
done
EOBJS=
for u in $STEPENC_UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    EOBJS="$EOBJS $obj"
done
POBJS=
for u in $POLICY_UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    POBJS="$POBJS $obj"
done
LOBJS=
for u in $LEARN_UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    LOBJS="$LOBJS $obj"
done
ROBJS=
for u in $RETURNS_UNITS; do
    src=${u%%:*}; obj=../build/${src%.*}.o
    hipcc $F ${u##*:} -c $src -o $obj
    ROBJS="$ROBJS $obj"
done
hipcc --offload-arch=gfx950 -shared $NOBJS -o ../librogue_gym_novelty.so
hipcc --offload-arch=gfx950 -shared $AOBJS -o ../librogue_gym_archive.so
hipcc --offload-arch=gfx950 -shared $FOBJS -o ../librogue_gym_obsfix.so
hipcc --offload-arch=gfx950 -shared $EOBJS -o ../librogue_gym_stepenc.so
hipcc --offload-arch=gfx950 -shared $POBJS -o ../librogue_gym_policy.so
hipcc --offload-arch=gfx950 -shared $LOBJS -o ../librogue_gym_learn.so
hipcc --offload-arch=gfx950 -shared $ROBJS -o ../librogue_gym_returns.so
hipcc --offload-arch=gfx950 -shared $OBJS -L.. -lrogue_gym_novelty -lrogue_gym_archive -lrogue_gym_obsfix -lrogue_gym_stepenc -lrogue_gym_policy -lrogue_gym_learn -lrogue_gym_returns '-Wl,-rpath,$ORIGIN' -o "$OUT"
echo "built $OUT"
