#!/bin/bash
# AddressSanitizer + UBSan run of the UFBoot split / support / consensus functions (iq-tree_amd/host/ufboot_splits.h) as a
# stand-alone program on the CPU: no device, nothing loaded into Python.
set -e
cd "$(dirname "$0")/.."
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -o "$D/asan_ufboot_splits" tools/asan_ufboot_splits.cpp
"$D/asan_ufboot_splits"
