#!/bin/bash
# gecm_parse_resume_line_method and gecm_resume_line_std_bound_method of libgecm under AddressSanitizer + UBSan (CPU only;
# a program of its own).
set -e
cd "$(dirname "$0")/.."
H=avx-ecm_amd/host
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
gcc -O1 -g -std=gnu11 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -Wall -Wextra tools/unit_sanitize.c $H/gecm_resume.c $H/mpl.c $H/gecm_mod.c $H/gecm_plan.c -lpthread -lm -o "$tmp/gecm_unit_sanitize"
ASAN_OPTIONS=detect_leaks=1 "$tmp/gecm_unit_sanitize"
