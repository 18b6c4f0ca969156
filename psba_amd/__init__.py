"""psba_amd -- MI355X-native Schur-complement bundle-adjustment normal-equations path.

The product is the HIP C-ABI library ``psba_amd/libpsba_hip.so`` (include/psba_hip.h).  This
package is only a ctypes binding to it for tests, bench.py and Python callers.  There is no CPU
fallback: importing :mod:`psba_amd.capi` raises if the library has not been built, and creating
a handle raises if no GPU is present.
"""
from .capi import (Psba, PsbaError, Problem, lib, lib_path, read_problem, partition_points,  # noqa: F401
                   write_problem, convert_bal, read_problem_ex, convert_bal_kd,
                   LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY, LOSS_SOFT_L1,
                   CAMERA_FIXED_K, CAMERA_FREE_K, CAMERA_FREE_KD, INTRINSICS_BAL,
                   DAMPING_IDENTITY, DAMPING_MARQUARDT, SOLVER_DENSE, SOLVER_PCG, SOLVER_SPARSE, PSBA_OK, PSBA_NOT_SPD, PSBA_SINGULAR_V)

__all__ = ["Psba", "PsbaError", "Problem", "lib", "lib_path", "read_problem", "partition_points",
           "write_problem", "convert_bal", "read_problem_ex", "convert_bal_kd",
           "LOSS_NONE", "LOSS_HUBER", "LOSS_CAUCHY", "LOSS_SOFT_L1",
           "CAMERA_FIXED_K", "CAMERA_FREE_K", "CAMERA_FREE_KD", "INTRINSICS_BAL",
           "DAMPING_IDENTITY", "DAMPING_MARQUARDT", "SOLVER_DENSE", "SOLVER_PCG", "SOLVER_SPARSE",
           # statuses of Psba.covariance (camera_covariance, covariance_matrix and point_covariance are its getters)
           "PSBA_OK", "PSBA_NOT_SPD", "PSBA_SINGULAR_V"]
