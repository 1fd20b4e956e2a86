#!/bin/bash
# AddressSanitizer + UBSan run of the partition-file parser and site extractor (iq-tree_amd/host/partition_spec.h) as a
# stand-alone program on the CPU: no device, nothing loaded into Python.
set -e
cd "$(dirname "$0")/.."
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -o "$D/asan_partition_spec" tools/asan_partition_spec.cpp
"$D/asan_partition_spec"
