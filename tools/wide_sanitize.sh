#!/bin/bash
# The host side of a wide context (gecm_mod.c: the wide limb rule, the row kernel's constants at 41, 44 and 48 rows, raw
# limbs -> canonical -> plain -> gcd) under AddressSanitizer + UBSan (CPU only; a program of its own).
set -e
cd "$(dirname "$0")/.."
H=avx-ecm_amd/host
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
gcc -O1 -g -std=gnu11 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -Wall -Wextra tools/wide_sanitize.c $H/mpl.c $H/gecm_mod.c -lpthread -lm -o "$tmp/gecm_wide_sanitize"
ASAN_OPTIONS=detect_leaks=1 "$tmp/gecm_wide_sanitize"
