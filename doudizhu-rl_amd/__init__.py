"""doudizhu-rl_amd: MI355X-native batched Doudizhu environment (hot path of
charleschen003/doudizhu-rl: deal, legal-move enumeration, action application,
terminal/reward, state encoding).  HIP kernels + C ABI under csrc/, host mirror of the
reference's envi.py here.  Import never touches the GPU; using the engine without the
built library or without an MI355X raises (there is no CPU fallback)."""
from ._lib import DdzError  # noqa: F401
from .engine import (BatchedEnv, GuidedSearch, PlayoutLeaf, guided_values, puct_priors, FACE_PLANES, NUM_ACTIONS, STEP_CHOICE, STEP_IDS, STEP_RANDOM,  # noqa: F401
                     STEP_ROWS, TRAJ_BYTES, TRAJ_PACKED_BYTES, action_table, auto_choose, cards_value, get_moves, get_moves_slab,
                     pack_trajectory, q_features, q_features_needed, q_first_fwd, q_first_bwd, q_stage_fwd, q_stage_bwd, q_fc1_dense, q_fc1_rows, q_fc1_rows_k,
                     q_features_rows, q_features_drows, q_gather_h0, q_shared_ws_bytes, q_shared_need_ws_bytes,
                     q_roles_ws_bytes, q_roles_need_ws_bytes, rows_to_onehot, state_prob, observe_states, tr_ws_bytes,
                     tr_ring_bytes, tr_ring_layout, mc_ws_bytes, mc_ws_layout, mc_ring_bytes,
                     mc_ring_layout, teach_ws_bytes, teach_ws_layout, Teacher, TeacherStats,
                     STATUS_MISMATCH, STATUS_CAPACITY, STATUS_BAD_LAST, STATUS_AUTO_WAIT, STATUS_AUTO_DEPTH, STATUS_Q_NO_ROW,
                     STATUS_DOMAIN, STATUS_CFR_CAPACITY, STATUS_SOLVE_DEPTH)
from .dqn_glue import (PackedBatch, QLeaf, ReturnBatch, ReturnRecorder, RoleQ, SeatLoop, TeacherAssembler, TeacherRecorder,  # noqa: F401
                       TrainLoop, TransitionRecorder, compete, mc_step, train)
from .envi import Env, EnvComplicated, EnvCooperation, EnvCooperationSimplify  # noqa: F401
