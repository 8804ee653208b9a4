"""MI355X-native scan-to-map ICP path for open3d_slam / libpointmatcher (C ABI: include/o3s_icp.h)."""
from .icp import (ICP, IcpConfig, IcpStats, ConvergenceError, TransformationError, InvalidModuleType, HipError,  # noqa: F401
                  compute_batch)
from .dense_map import DenseMap  # noqa: F401
from .submap import AssembledMap, ProcessedScan, Submap  # noqa: F401
from .submap_collection import SubmapCollection  # noqa: F401
from .odometry import ConstantVelocityMotionCompensation, LidarOdometry, RawScan, TransformBuffer  # noqa: F401
from .pose_graph import Constraint, OptimizationProblem, loop_closure_step, update_submaps_and_trajectory  # noqa: F401
from .constraint_builders import build_odometry_constraint, compute_odometry_constraints  # noqa: F401
from .place_recognition import PlaceRecognition, PlaceRecognitionParameters  # noqa: F401
from .pose_search import PoseSearchParams, PoseSearchResult, LocalizeResult, localize  # noqa: F401
from . import pose_search  # noqa: F401  (pose_search.search / pose_search.pose)

__all__ = ["ICP", "IcpConfig", "IcpStats", "ConvergenceError", "TransformationError", "InvalidModuleType", "HipError", "compute_batch", "Submap", "AssembledMap", "ProcessedScan", "SubmapCollection", "DenseMap", "LidarOdometry",
           "ConstantVelocityMotionCompensation", "TransformBuffer", "RawScan", "Constraint", "OptimizationProblem", "update_submaps_and_trajectory", "loop_closure_step", "build_odometry_constraint", "compute_odometry_constraints",
           "PlaceRecognition", "PlaceRecognitionParameters", "PoseSearchParams", "PoseSearchResult", "LocalizeResult", "localize", "pose_search"]
