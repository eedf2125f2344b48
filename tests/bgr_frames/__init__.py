"""GPU tests of ffgpu_exec_forward_bgr_frames_dev (mixed-size u8 frame batches)."""
