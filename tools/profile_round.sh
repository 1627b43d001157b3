#!/bin/bash
# usage (GPU machine): tools/profile_round.sh <tag> <stage>   stages: tests | bench | prof | trace (tools/profile_round.py says what each records)
exec python3 "$(dirname "$0")/profile_round.py" "$@"
