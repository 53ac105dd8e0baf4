'''
MI355X dense simplex pivot engine behind the lpsol Tableau/Simplex API
(reference: tkoz0/linear-program-solver, lpsol/__init__.py:5-17).
'''

from .tableau import Tableau
from .simplex import Simplex
from .linprog import LinProg
from ._lib import Engine, BatchEngine, EngineUnavailable, DeviceError
from ._lib import RULE_STANDARD, RULE_MIN_INDEX, RULE_MAX_INCREASE, RULE_DUAL
from .batch import solve_batch, BatchResult, solve_lp_batch, LPBatchResult
from .batch import solve_ragged, RaggedResult, solve_lp_ragged, LPRaggedResult
from .batch import solution_x
from .problem import solve_problems, ProblemResult, solve_problems_ragged, ProblemRaggedResult
from .problem import problem_columns, assemble_tableaux, problem_duals, pack_problems
from .problem import general_kinds, general_shape, pack_general, general_standard_form, general_recover, general_duals
from .problem import extend_tableau
from ._lib import VAR_PLAIN, VAR_LOWER, VAR_BOXED, VAR_UPPER, VAR_FREE

__all__ = [
    'solve_problems',
    'ProblemResult',
    'solve_problems_ragged',
    'ProblemRaggedResult',
    'problem_columns',
    'assemble_tableaux',
    'problem_duals',
    'pack_problems',
    'general_kinds',
    'general_shape',
    'pack_general',
    'general_standard_form',
    'general_recover',
    'general_duals',
    'extend_tableau',
    'VAR_PLAIN',
    'VAR_LOWER',
    'VAR_BOXED',
    'VAR_UPPER',
    'VAR_FREE',
    'Tableau',
    'Simplex',
    'LinProg',
    'Engine',
    'BatchEngine',
    'solve_batch',
    'BatchResult',
    'solve_lp_batch',
    'LPBatchResult',
    'solve_ragged',
    'RaggedResult',
    'solve_lp_ragged',
    'LPRaggedResult',
    'solution_x',
    'EngineUnavailable',
    'DeviceError',
    'RULE_STANDARD',
    'RULE_MIN_INDEX',
    'RULE_MAX_INCREASE',
    'RULE_DUAL',
]
