// (dim_x, dim_u, order) shapes with compiled kernels; parsed by build.py and included by m4q_capi.hip.
// A line that ends in "plant-only" is compiled with -DM4Q_PLANT_ONLY: plant_kernel and the plant rollouts alone
// (m4q_plant_step_batch, ...) - the two-qubit plant under two controls of the reference's crosstalk scenario
// (tests/test_mpc4quantum.py:281-397) as a one-shot entry; the 21 closed-loop kernels of (16, 2, 1) were 3.3 MB nobody could launch.
// That scenario's closed loop runs on the reduced (8, 2, 1) model and stays on the device as an OBSERVED PLANT (m4q_observe.h): the
// (8, 2, 1) object holds the complex closed-loop kernels and observed_plant_kernel<PARTIAL_TRACE>, which steps the joint 16-entry
// state itself; the dim_x = 4 objects hold observed_plant_kernel<QUBIT_BLOCK>, the 9-entry leaky transmon behind a qubit model.
// (16, 1, 1-4): a single-qubit gate's process vector (n = 2^4, one drive; the reference's TestGateSynth.test_NOT_gate,
// tests/test_mpc4quantum.py:47-145, loops over orders 1-4) - also a d = 4 density matrix under one drive.  Orders 3 and 4 have no
// device discretisation (discretize_kernel: orders 1-2): their models come from the host.
M4Q_SHAPE(4, 1, 1)
M4Q_SHAPE(4, 1, 2)
M4Q_SHAPE(4, 2, 1)
M4Q_SHAPE(9, 2, 1)
M4Q_SHAPE(9, 2, 2)
M4Q_SHAPE(16, 3, 1)
M4Q_SHAPE(16, 1, 1)
M4Q_SHAPE(16, 1, 2)
M4Q_SHAPE(16, 1, 3)
M4Q_SHAPE(16, 1, 4)
M4Q_SHAPE(8, 2, 1)
M4Q_SHAPE(16, 2, 1)   // plant-only
