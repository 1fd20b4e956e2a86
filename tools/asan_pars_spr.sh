#!/bin/bash
# AddressSanitizer + UBSan run of the SPR scan's host-side validation (iq-tree_amd/csrc/pars_spr_check.h) as a stand-alone
# program on the CPU: no device, nothing loaded into Python.
set -e
cd "$(dirname "$0")/.."
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -o "$D/asan_pars_spr_check" tools/asan_pars_spr_check.cpp
"$D/asan_pars_spr_check"
