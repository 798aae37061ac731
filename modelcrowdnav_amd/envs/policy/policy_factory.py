"""Name -> policy constructor table (reference: crowd_sim/envs/policy/policy_factory.py:1-12)."""
from .linear import Linear
from .orca import ORCA
from .socialforce import SocialForce

policy_factory = {"linear": Linear, "orca": ORCA, "socialforce": SocialForce, "none": lambda: None}
