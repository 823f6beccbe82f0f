"""Command-line entry points (reference src/lesion_gnn/scripts)."""
