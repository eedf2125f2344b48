"""GPU tests of ffgpu_exec_forward_nv12_frames_dev (mixed-size NV12 frame batches)."""
