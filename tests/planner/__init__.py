"""GPU tests of the executor planner: the plans of the repo's cfgs, pinned (tools/plan_pin.py, tests/data/plan_pin.json)."""
