"""Robot policy table (reference: crowd_nav/policy/policy_factory.py:1-8)."""
from ..envs.policy.policy_factory import policy_factory
from .cadrl import CADRL
from .lstm_rl import LstmRL
from .sarl import SARL

policy_factory["cadrl"] = CADRL
policy_factory["lstm_rl"] = LstmRL
policy_factory["sarl"] = SARL
