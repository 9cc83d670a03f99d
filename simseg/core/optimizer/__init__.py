"""`simseg.core.optimizer`: the name the reference's configs resolve `optim.name: LARS` through (core/hooks/optimizer.py:103-115 evaluates
the bare name after `from simseg.core.optimizer import *`).  The optimizer itself is the table-driven HIP one."""
from simseg_amd.optim import LARS

__all__ = ["LARS"]
