"""MI355X-native batched fast-SLS QP path.  Public names re-exported here."""
from .models import ModelData, pendulum, quadrotor, rocket, get_model, plant_param_names, plant_param_defaults, pack_plant_params  # noqa: F401
from .bounds import pack_bounds, box_bounds, bounds_window, constraint_margin  # noqa: F401,E402
from ._lib import X0_BOX_TOL_OSQP_DEFAULT  # noqa: F401,E402
from .fast_sls import BatchedFastSLS, fast_SLS  # noqa: F401,E402
from .synthetic import make_batch  # noqa: F401,E402
from .closed_loop import ClosedLoopMPC  # noqa: F401,E402
from .monte_carlo import run_monte_carlo, disturbance_stream, can_run_persistent, measurement_stream, meas_noise_table  # noqa: F401,E402
