"""Bill of materials as CSV (the reference's rendering/bom.py): a `name,count` header, then one row per BOM item --
its name, its count and the part's attributes."""
import csv


def render_bom(obj, filename):
    """Write `obj.bom()` (an assembly's recursive BOM) to `filename`."""
    with open(filename, "w", newline="") as f:
        writer = csv.writer(f)
        writer.writerow(["name", "count"])
        for item in obj.bom():
            writer.writerow([item.name, item.count] + list(item.part.attributes))
