"""Doppler shift of a moving source heard by a moving receiver (mirror of quantum_inferno/synth/doppler.py), behind the
reference's names and signatures.  The small helpers are host NumPy; the geometry of doppler_forward / doppler_inverse and their
image variants -- arrival or emission time, range and omega over omega_c for every sample -- is one kernel on the device
(engine.doppler, qi_doppler), every operation rounded as NumPy rounds it.  NumPy in, NumPy out.  For an array of receivers,
stack geometry_row's rows and call engine.doppler once."""
from typing import Tuple

import numpy as np
import torch

from .. import engine


def time_duration(time_vector: np.ndarray) -> float:
    """Largest minus smallest time."""
    return np.max(time_vector) - np.min(time_vector)


def time_4d_mx(time_array: np.ndarray, space_dimensions: int) -> np.array:
    """[time] -> [time, space_dimensions]: every column the times."""
    return np.array([time_array, ] * space_dimensions).transpose()


def space_4d_mx(space_column_vector: np.ndarray, time_number_samples: int) -> np.array:
    """[xyz] -> [time_number_samples, xyz]: every row the vector."""
    return np.array([space_column_vector, ] * time_number_samples)


def hadamard_dot_product_mx(x_mx: np.ndarray, y_mx: np.ndarray) -> np.ndarray:
    """Row-wise dot product of two [time, xyz] matrices."""
    return np.sum(x_mx * y_mx, 1)


def range_vector_sr(x_initial_position_vector: np.array, x_final_position_vector: np.array) -> np.array:
    """Vector from the first position to the second."""
    return x_final_position_vector - x_initial_position_vector


def range_matrix_sr(x_source_mx: np.ndarray, x_receiver_mx: np.ndarray) -> np.ndarray:
    """Receiver minus source, [time, xyz]."""
    return x_receiver_mx - x_source_mx


def range_hadamard(r_mx: np.ndarray) -> np.ndarray:
    """Length of every row of a [time, xyz] matrix."""
    return np.sqrt(hadamard_dot_product_mx(r_mx, r_mx))


def range_scalar(x_source_vector: np.array, x_receiver_vector: np.array) -> float:
    """Distance between two positions."""
    range_vector = range_vector_sr(x_source_vector, x_receiver_vector)
    return np.sqrt(np.sum(range_vector * range_vector))


def _velocity(speed_mps: float, position_vector_init_xyz_m, position_vector_final_xyz_m) -> np.ndarray:
    """The velocity vector: the speed along the unit vector of the trajectory, zeros for an object at rest."""
    if speed_mps > 0:
        trajectory_m = range_scalar(position_vector_init_xyz_m, position_vector_final_xyz_m)
        return speed_mps * (range_vector_sr(position_vector_init_xyz_m, position_vector_final_xyz_m) / trajectory_m)
    return np.zeros(3)


def geometry_row(signal_speed_mps, source_speed_mps, receiver_speed_mps, source_position_vector_initial_xyz_m,
                 source_position_vector_final_xyz_m, receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m,
                 inverse: bool = False) -> np.ndarray:
    """The parameter row of engine.doppler for one source and receiver: c, c**2, 1. / (c**2 - speed**2) -- the receiver's speed
    forward, the source's inverse -- the two velocity vectors and the initial range, each by the reference's expression."""
    positions = [np.asarray(v, dtype=np.float64) for v in (source_position_vector_initial_xyz_m, source_position_vector_final_xyz_m,
                                                           receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m)]
    if any(v.shape != (3,) for v in positions):
        raise ValueError("positions must be 3-element XYZ vectors")
    object_speed_mps = source_speed_mps if inverse else receiver_speed_mps
    denom = 1. / (signal_speed_mps**2 - object_speed_mps**2)
    return np.concatenate([[signal_speed_mps, signal_speed_mps**2, denom], _velocity(source_speed_mps, positions[0], positions[1]),
                           _velocity(receiver_speed_mps, positions[2], positions[3]), positions[2] - positions[0]]).astype(np.float64)


def _doppler(times_s, row, inverse) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    if np.ndim(times_s) != 1 or np.size(times_s) < 1:
        raise ValueError(f"the times must be a record [n], got shape {tuple(np.shape(times_s))}")
    outs = engine.doppler(row, len(times_s), ("timestamps", times_s), inverse=inverse)
    host = torch.stack(outs).cpu().numpy()  # one copy
    return host[0], host[1], host[2]


def _space(space_dimensions: int):
    if space_dimensions != 3:
        raise ValueError(f"space_dimensions must be 3 to match the XYZ position vectors, got {space_dimensions}")


def doppler_forward(tau_source_s, signal_speed_mps, source_speed_mps, receiver_speed_mps, space_dimensions,
                    source_position_vector_initial_xyz_m, source_position_vector_final_xyz_m,
                    receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m
                    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Source times -> (receiver times in seconds, range in metres, omega over omega_c)."""
    _space(space_dimensions)
    row = geometry_row(signal_speed_mps, source_speed_mps, receiver_speed_mps, source_position_vector_initial_xyz_m,
                       source_position_vector_final_xyz_m, receiver_position_vector_initial_xyz_m,
                       receiver_position_vector_final_xyz_m, inverse=False)
    return _doppler(tau_source_s, row, False)


def image_doppler_forward(tau_source_s, signal_speed_mps, source_speed_mps, receiver_speed_mps, space_dimensions,
                          source_position_vector_initial_xyz_m, source_position_vector_final_xyz_m,
                          receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m
                          ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """doppler_forward for the source mirrored at the plane z = 0."""
    mirror = np.array([1., 1., -1.])
    return doppler_forward(tau_source_s, signal_speed_mps, source_speed_mps, receiver_speed_mps, space_dimensions,
                           source_position_vector_initial_xyz_m * mirror, source_position_vector_final_xyz_m * mirror,
                           receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m)


def doppler_inverse(inv_time_receiver_s, signal_speed_mps, source_speed_mps, receiver_speed_mps, space_dimensions,
                    source_position_vector_initial_xyz_m, source_position_vector_final_xyz_m,
                    receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m
                    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Receiver times -> (source times in seconds, range in metres, omega over omega_c)."""
    _space(space_dimensions)
    row = geometry_row(signal_speed_mps, source_speed_mps, receiver_speed_mps, source_position_vector_initial_xyz_m,
                       source_position_vector_final_xyz_m, receiver_position_vector_initial_xyz_m,
                       receiver_position_vector_final_xyz_m, inverse=True)
    return _doppler(inv_time_receiver_s, row, True)


def image_doppler_inverse(inv_time_receiver_s, signal_speed_mps, source_speed_mps, receiver_speed_mps, space_dimensions,
                          source_position_vector_initial_xyz_m, source_position_vector_final_xyz_m,
                          receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m
                          ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """doppler_inverse for the source mirrored at the plane z = 0."""
    mirror = np.array([1., 1., -1.])
    return doppler_inverse(inv_time_receiver_s, signal_speed_mps, source_speed_mps, receiver_speed_mps, space_dimensions,
                           source_position_vector_initial_xyz_m * mirror, source_position_vector_final_xyz_m * mirror,
                           receiver_position_vector_initial_xyz_m, receiver_position_vector_final_xyz_m)
