"""The record layouts of include/uflow_frame_codec.h, include/uflow_flush_ctl.h and include/uflow_route.h, declared
once for Python.

Every batched call takes and returns arrays of these records: numpy structured arrays on the host
(uflow_amd.frame), uint8[n, itemsize] rows on the device (uflow_amd.batch.rows / records).  FOO_BAR_DTYPE is the C
struct ufc_foo_bar, field for field; RECORDS maps the struct names to the dtypes.  tests/test_records_cpu.py compiles
sizeof and offsetof of every struct and field from the header and compares them with this table, so a layout is
written here and nowhere else.  numpy only: no ctypes, no torch.
"""
import numpy as np

# numpy views of ufc_frame_info / ufc_item (batched outputs)
FRAME_INFO_DTYPE = np.dtype([("kind", "u1"), ("ok", "u1"), ("aux", "u1"), ("crc_ok", "u1"), ("f", "<u4", (5,)),
                             ("item_count", "<u4"), ("item_first", "<u4")])
ITEM_DTYPE = np.dtype([("id", "<u4"), ("channel_id", "u1"), ("form", "u1"), ("window_parent_lead", "<u2"),
                       ("channel_parent_lead", "<u2"), ("fragment_id", "<u2"), ("fragment_id_last", "<u2"),
                       ("flags", "<u2"), ("data_offset", "<u4"), ("data_len", "<u4")])
# ufc_flush / ufc_flush_result (batched packs)
FLUSH_DTYPE = np.dtype([("flush_alloc", "<i8"), ("kind", "<u4"), ("window_room", "<u4"), ("id0", "<u4"), ("id1", "<u4")])
FLUSH_RESULT_DTYPE = np.dtype([("frame_first", "<u4"), ("frame_count", "<u4"), ("items_packed", "<u4"), ("stop", "<u4"),
                               ("alloc_left", "<i8")])
# ufc_packet / ufc_sender / ufc_packet_result / ufc_sender_result (batched packet emits)
PACKET_DTYPE = np.dtype([("data_offset", "<u4"), ("data_len", "<u4"), ("flush_id", "<u4"), ("channel_id", "u1"),
                         ("mode", "u1"), ("reserved", "<u2")])
SENDER_DTYPE = np.dtype([("base_id", "<u4"), ("next_id", "<u4"), ("window_size", "<u4"), ("flush_id", "<u4"),
                         ("alloc", "<u8"), ("max_alloc", "<u8"), ("window_parent_id", "<u4"), ("take", "<u4"),
                         ("reserve_items", "<u4"), ("reserved", "<u4"), ("channel_parent_id", "<u4", (64,))])
PACKET_RESULT_DTYPE = np.dtype([("sequence_id", "<u4"), ("item_first", "<u4"), ("item_count", "<u4"), ("status", "u1"),
                                ("resend", "u1"), ("reserved", "<u2")])
SENDER_RESULT_DTYPE = np.dtype([("item_first", "<u4"), ("item_count", "<u4"), ("packets_consumed", "<u4"),
                                ("packets_emitted", "<u4"), ("packets_dropped", "<u4"), ("stop", "<u4"),
                                ("bytes_dropped", "<u8")])
# ufc_receiver / ufc_rx_slot / ufc_rx_packet / ufc_receiver_result (batched packet receives)
RECEIVER_DTYPE = np.dtype([("base_id", "<u4"), ("end_id", "<u4"), ("window_size", "<u4"), ("window_ready", "u1"),
                           ("deliver", "u1"), ("reserved", "<u2"), ("resync_id", "<u4"), ("reserved2", "<u4"),
                           ("alloc", "<u8"), ("max_alloc", "<u8"), ("channel_ready_flags", "<u8"),
                           ("channel_base_id", "<u4", (64,)), ("channel_packet_count", "<u4", (64,))])
RX_SLOT_DTYPE = np.dtype([("data_offset", "<u8"), ("data_len", "<u4"), ("asm_size", "<u4"),
                          ("asm_window_parent_lead", "<u2"), ("asm_channel_parent_lead", "<u2"),
                          ("asm_last_fragment_id", "<u2"), ("asm_received", "<u2"), ("rx_window_parent_lead", "<u2"),
                          ("rx_channel_parent_lead", "<u2"), ("asm_state", "u1"), ("asm_channel_id", "u1"),
                          ("rx_channel_id", "u1"), ("rx_flags", "u1")])
RX_PACKET_DTYPE = np.dtype([("out_offset", "<u8"), ("sequence_id", "<u4"), ("len", "<u4"), ("channel_id", "u1"),
                            ("flags", "u1"), ("reserved", "<u2"), ("reserved2", "<u4")])
RECEIVER_RESULT_DTYPE = np.dtype([("packet_first", "<u4"), ("packet_count", "<u4"), ("status_count", "<u4", (11,)),
                                  ("packets_completed", "<u4"), ("packets_dud", "<u4"), ("advanced", "<u4"),
                                  ("stop", "<u4"), ("reserved", "<u4"), ("bytes_delivered", "<u8")])
# ufc_frame_window / ufc_frame_window_result (batched frame windows)
FRAME_WINDOW_DTYPE = np.dtype([("base_id", "<u4"), ("size", "<u4"), ("tail_base_id", "<u4"), ("tail_bitfield", "<u4"),
                               ("tail_nonce", "u1"), ("has_tail", "u1"), ("sync_reply", "u1"), ("reserved", "u1"),
                               ("reserved2", "<u4")])
FRAME_WINDOW_RESULT_DTYPE = np.dtype([("group_first", "<u4"), ("group_count", "<u4"), ("accepted", "<u4"),
                                      ("refused", "<u4"), ("syncs", "<u4"), ("packet_syncs", "<u4"),
                                      ("first_packet_sync", "<u4"), ("advanced", "<u4"), ("stop", "<u4"),
                                      ("reserved", "<u4")])
# ufc_sent_frame / ufc_frame_queue / ufc_frame_queue_step / ufc_frame_queue_result (batched sender frame queues)
SENT_FRAME_DTYPE = np.dtype([("send_time_ms", "<u8"), ("size", "<u4"), ("ref_first", "<u4"), ("ref_count", "<u4"),
                             ("flags", "u1"), ("reserved", "u1", (3,))])
FRAME_QUEUE_DTYPE = np.dtype([("log_base_id", "<u4"), ("log_next_id", "<u4"), ("window_base_id", "<u4"),
                              ("window_size", "<u4"), ("tail_size", "<u4"), ("rb_base_id", "<u4"), ("rb_max_span", "<u4"),
                              ("rb_frames", "<u4", (2,)), ("rb_count", "<u4"), ("rate_limited", "u1"),
                              ("has_ack_data", "u1"), ("ack_rate_limited", "u1"), ("has_last_feedback", "u1"),
                              ("li_count", "<u4"), ("ack_last_send_time_ms", "<u8"), ("ack_total_size", "<u8"),
                              ("last_feedback_ms", "<u8"), ("li_end_time_ms", "<u8", (9,)), ("li_length", "<u4", (9,)),
                              ("log_cap", "<u4"), ("log_first", "<u8")])
FRAME_QUEUE_STEP_DTYPE = np.dtype([("flags", "<u4"), ("reserved", "<u4"), ("rtt_ms", "<u8"), ("thresh_ms", "<u8"),
                                   ("now_ms", "<u8"), ("reset_loss_rate", "<f8")])
FRAME_QUEUE_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("pushes_taken", "<u4"), ("pushes_refused", "<u4"),
                                     ("ack_frames", "<u4"), ("groups", "<u4"), ("groups_dud", "<u4"),
                                     ("groups_unknown", "<u4"), ("groups_bad_nonce", "<u4"), ("frames_acked", "<u4"),
                                     ("li_acks", "<u4"), ("li_nacks", "<u4"), ("window_advanced", "<u4"),
                                     ("log_culled", "<u4"), ("window_room", "<u4"), ("has_feedback", "u1"),
                                     ("rate_limited", "u1"), ("reserved", "<u2"), ("receive_rate", "<u4"),
                                     ("rtt_ms", "<u8"), ("loss_rate", "<f8")])
# ufc_recv_rate_entry / ufc_rate_state / ufc_rate_tick / ufc_rate_result (batched send rate control)
RECV_RATE_ENTRY_DTYPE = np.dtype([("timestamp_ms", "<u8"), ("value", "<u4"), ("is_initial", "u1"),
                                  ("reserved", "u1", (3,))])
RATE_STATE_DTYPE = np.dtype([("mode", "<u4"), ("send_rate", "<u4"), ("max_send_rate", "<u4"), ("send_rate_tcp", "<u4"),
                             ("has_time_last_doubled", "u1"), ("has_nofeedback_exp", "u1"), ("nofeedback_idle", "u1"),
                             ("has_rtt_s", "u1"), ("has_rtt_ms", "u1"), ("has_rto_ms", "u1"), ("has_last_flush", "u1"),
                             ("has_reset", "u1"), ("time_last_doubled_ms", "<u8"), ("prev_loss_rate", "<f8"),
                             ("nofeedback_exp_ms", "<u8"), ("rtt_s", "<f8"), ("rtt_ms", "<u8"), ("rto_ms", "<u8"),
                             ("now_ms", "<u8"), ("flush_alloc", "<i8"), ("reset_loss_rate", "<f8"),
                             ("recv_first", "<u8"), ("recv_count", "<u4"), ("recv_cap", "<u4")])
RATE_TICK_DTYPE = np.dtype([("now_ms", "<u8"), ("delta_time_s", "<f8"), ("alloc_adjust", "<i8"), ("flags", "<u4"),
                            ("reserved", "<u4")])
RATE_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("mode", "<u4"), ("now_ms", "<u8"), ("rtt_ms", "<u8"), ("rto_ms", "<u8"),
                              ("flush_alloc", "<i8"), ("send_rate", "<u4"), ("flags", "<u4"), ("inv_iterations", "<u4"),
                              ("recv_count", "<u4")])
# ufc_resend_entry / ufc_sent_packet / ufc_tx_ref / ufc_resend / ufc_resend_result / ufc_resend_commit_result
RESEND_ENTRY_DTYPE = np.dtype([("resend_time_ms", "<u8"), ("sequence_id", "<u4"), ("fragment_id", "<u2"),
                               ("send_count", "u1"), ("reserved", "u1")])
SENT_PACKET_DTYPE = np.dtype([("data_offset", "<u4"), ("data_len", "<u4"), ("frag_first", "<u4"), ("sequence_id", "<u4"),
                              ("window_parent_lead", "<u2"), ("channel_parent_lead", "<u2"), ("channel_id", "u1"),
                              ("resend", "u1"), ("reserved", "<u2")])
TX_REF_DTYPE = np.dtype([("sequence_id", "<u4"), ("fragment_id", "<u2"), ("flags", "<u2")])
RESEND_DTYPE = np.dtype([("heap_first", "<u8"), ("heap_cap", "<u4"), ("heap_len", "<u4"), ("pkt_first", "<u8"),
                         ("pkt_cap", "<u4"), ("frag_next", "<u4"), ("frag_first", "<u8"), ("frag_cap", "<u4"),
                         ("tx_cap", "<u4"), ("tx_first", "<u8"), ("tx_head", "<u4"), ("tx_tail", "<u4"),
                         ("stage_first", "<u8"), ("stage_cap", "<u4"), ("pending_seq", "<u4"), ("pending_next", "<u4"),
                         ("pending_count", "<u4"), ("pending_resend", "u1"), ("reserved0", "u1"), ("reserved1", "<u2"),
                         ("reserved2", "<u4"), ("window_bytes", "<u8")])
RESEND_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("n_resent", "<u4"), ("n_pending_staged", "<u4"),
                                ("heap_popped_dead", "<u4"), ("heap_popped_acked", "<u4"), ("packets_freed", "<u4"),
                                ("refs_acked", "<u4"), ("heap_len", "<u4"), ("pending_count", "<u4"),
                                ("acks_ignored", "<u4"), ("bytes_freed", "<u8")])
RESEND_COMMIT_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("pending_packed", "<u4"), ("packets_entered", "<u4"),
                                       ("heap_pushed", "<u4"), ("heap_dropped", "<u4"), ("refs_written", "<u4"),
                                       ("frames", "<u4"), ("take", "<u4"), ("heap_len", "<u4"), ("pending_count", "<u4")])

# C struct name -> dtype (ufc_item -> ITEM_DTYPE, ...).
RECORDS = {"ufc_" + k[:-len("_DTYPE")].lower(): v for k, v in list(globals().items()) if k.endswith("_DTYPE")}

# include/uflow_flush_ctl.h, the header of the batched flush control, has a table of its own (tests/test_flush_cpu.py
# holds it to that header as tests/test_records_cpu.py holds RECORDS to uflow_frame_codec.h).
# ufc_flush_ctl / ufc_flush_acks_result / ufc_flush_sync_result (batched flush control)
FLUSH_CTL_DTYPE = np.dtype([("sync_timeout_base_ms", "<u8"), ("keepalive_interval_ms", "<u8"), ("carry_first", "<u8"),
                            ("carry_cap", "<u4"), ("carry_count", "<u4"), ("has_keepalive", "u1"), ("reserved0", "u1"),
                            ("reserved1", "<u2"), ("reserved2", "<u4")])
FLUSH_ACKS_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("merged_first", "<u4"), ("merged_count", "<u4"), ("carried", "<u4"),
                                    ("dropped", "<u4"), ("dud", "u1"), ("reserved", "u1", (3,))])
FLUSH_SYNC_RESULT_DTYPE = np.dtype([("sent", "<u4"), ("reason", "<u4"), ("heap_len", "<u4"), ("pending_count", "<u4"),
                                    ("mode", "u1"), ("is_send_pending", "u1"), ("reserved", "<u2"),
                                    ("reserved2", "<u4")])
FLUSH_RECORDS = {"ufc_flush_ctl": FLUSH_CTL_DTYPE, "ufc_flush_acks_result": FLUSH_ACKS_RESULT_DTYPE,
                 "ufc_flush_sync_result": FLUSH_SYNC_RESULT_DTYPE}

# include/uflow_route.h, the header of the batched frame routing, has a table of its own as well
# (tests/test_route_cpu.py holds it to that header).
# ufc_addr / ufc_route_slot / ufc_route_result (batched frame routing)
ADDR_DTYPE = np.dtype([("ip", "u1", (16,)), ("port", "<u2"), ("family", "u1"), ("reserved", "u1"), ("flowinfo", "<u4"),
                       ("scope_id", "<u4"), ("reserved2", "<u4")])
ROUTE_SLOT_DTYPE = np.dtype([("key", ADDR_DTYPE), ("conn", "<u4"), ("used", "u1"), ("reserved", "u1", (11,))])
ROUTE_RESULT_DTYPE = np.dtype([("frames", "<u4"), ("first_control", "<u4"), ("deferred", "<u4"), ("reserved", "<u4")])
ROUTE_RECORDS = {"ufc_addr": ADDR_DTYPE, "ufc_route_slot": ROUTE_SLOT_DTYPE, "ufc_route_result": ROUTE_RESULT_DTYPE}
