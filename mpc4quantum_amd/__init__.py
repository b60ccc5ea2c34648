"""mpc4quantum_amd - MI355X-native engine for the MPC hot path of andgoldschmidt/MPC4quantum.

Same public names as the reference package (mpc4quantum/__init__.py:3-7 star-exports experiment,
linearize, model, mpc, vectorize), backed by hand-written HIP kernels in libm4q_hip.so."""
from .exit_condition import QuadraticExit  # noqa: F401
from .experiment import (Experiment, LExperiment, QCoupledExperiment, QExperiment, QExperiment32, QSynthesis,  # noqa: F401
                         isqrt, plant_step_batch, process_dim, split_blocks)
from .feedback import (FeedbackLaw, model_feedback_batch, model_feedback_reference, plant_feedback_batch,  # noqa: F401
                       plant_feedback_reference)
from .fit import dmdc_fit_batch, dmdc_fit_qr_reference, dmdc_fit_reference, refit_models_batch, train_models_batch  # noqa: F401
from .grad import (model_rollout_grad_batch, model_rollout_grad_reference, ordered_weighted_sum,  # noqa: F401
                   plant_rollout_grad_batch, plant_rollout_grad_reference)
from .library import (create_library, create_library_from_list, create_power_list, diff_library, krtimes,  # noqa: F401
                      multinomial_powers, size_of_library)
from .linearize import WrapModel  # noqa: F401
from .model import DMDc, DiscrepDMDc, OnlineDMDc  # noqa: F401
from .noise import MeasurementNoise  # noqa: F401
from .online import online_dmdc_batch, online_dmdc_reference, stream_models_batch  # noqa: F401
from .mpc import (StepClock, complex_to_real, complex_to_real_op, iqp_line_search, isinf_warning, mpc, mpc_batch,  # noqa: F401
                  real_to_complex, real_to_complex_op, shift_guess, val_to_str)
from .optimize import quad_program, quad_program_batch  # noqa: F401
from .plant_linearize import plant_linearize_batch, plant_linearize_reference  # noqa: F401
from .plant_linearize import plant_quad_program_batch, plant_quad_program_reference  # noqa: F401
from .plant_param import (plant_calibrate_batch, plant_calibrate_reference, plant_param_grad_reference,  # noqa: F401
                          plant_param_op0, plant_rollout_param_grad_batch)
from .plant_sqp import plant_sqp_batch, plant_sqp_reference  # noqa: F401
from .plant_ilqr import plant_ilqr_batch, plant_ilqr_reference  # noqa: F401
from .plant_robust import (plant_robust_batch, plant_robust_reference, plant_rollout_multi_batch,  # noqa: F401
                           plant_rollout_multi_reference)
from .model_robust import (model_robust_batch, model_robust_reference, model_rollout_multi_batch,  # noqa: F401
                           model_rollout_multi_reference)
from .rollout import model_rollout_batch, plant_rollout_batch  # noqa: F401
from .session import EnsembleSession  # noqa: F401
from .vectorize import discretize_homogeneous, discretize_homogeneous_batch, liouvillian, vectorize_me  # noqa: F401

__version__ = "0.1.0"
