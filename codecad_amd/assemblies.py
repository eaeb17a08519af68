"""Assemblies: named parts placed by rigid transformations, and their bill of materials.

The modelling surface of the reference's assemblies (`codecad.assembly`, `Shape*.make_part`): a part is a
shape with a name and a list of attributes; an instance is a part (or a whole subassembly) with a rigid
transformation and a visibility flag; an assembly is a named list of instances of one dimension.  Instances
are immutable -- `translated*`, `rotated*` and `hidden` return new ones -- and scaling is not offered: an
assembly is a set of solid bodies.

The consumers take one shape, `asm.shape()`, the union of the visible instances; `interference()`
(interference.py) takes the assembly itself and evaluates every instance on its own.
"""
import collections

from . import util

_AXES = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1)}


class Part(collections.namedtuple("Part", "name data attributes")):
    """A named shape (`data`) with a list of attributes (extra BOM columns)."""

    __slots__ = ()


class Assembly(collections.namedtuple("Assembly", "name instances attributes")):
    """A named list of instances: PartTransform* or AssemblyTransform* of the same dimension."""

    __slots__ = ()


class _InstanceBase(collections.namedtuple("PartTransform", "part transform visible")):
    """A part (or an assembly) placed by `transform` (util.Transformation without scale)."""

    __slots__ = ()

    def shape(self):
        """The placed shape of this instance."""
        return self.part.data.transformed(self.transform)

    def _transformed(self, transform):
        # `transform` is applied after this instance's own one; callers only pass rigid transforms
        return self.__class__(self.part, transform * self.transform, self.visible)

    def hidden(self, hidden=True):
        """This instance hidden (or shown again with hidden=False): BOMs may skip it, shape() leaves it out."""
        return self.__class__(self.part, self.transform, not hidden)

    @property
    def name(self):
        return self.part.name

    @property
    def attributes(self):
        return self.part.attributes

    @staticmethod
    def _move(offset):
        return util.Transformation(util.Quaternion.zero(), util.Vector(*offset))

    @staticmethod
    def _turn(axis, angle):
        return util.Transformation(util.Quaternion.from_degrees(util.wrap_vector_like(axis), angle), util.Vector.zero())


class PartTransform2D(_InstanceBase):
    __slots__ = ()

    @staticmethod
    def dimension():
        return 2

    def translated(self, x, y=None):
        v = util.wrap_vector_like(x) if y is None else util.Vector(x, y)
        return self._transformed(self._move((v.x, v.y, 0)))

    def translated_x(self, distance):
        return self.translated(distance, 0)

    def translated_y(self, distance):
        return self.translated(0, distance)

    def rotated(self, angle):
        return self._transformed(self._turn((0, 0, 1), angle))


class PartTransform3D(_InstanceBase):
    __slots__ = ()

    @staticmethod
    def dimension():
        return 3

    def translated(self, x, y=None, z=None):
        if y is None and z is None:
            v = util.wrap_vector_like(x)
        elif y is not None and z is not None:
            v = util.Vector(x, y, z)
        else:
            raise ValueError("If y is specified, then z has to be too.")
        return self._transformed(self._move(v))

    def translated_x(self, distance):
        return self.translated(distance, 0, 0)

    def translated_y(self, distance):
        return self.translated(0, distance, 0)

    def translated_z(self, distance):
        return self.translated(0, 0, distance)

    def rotated(self, axis, angle):
        return self._transformed(self._turn(axis, angle))

    def rotated_x(self, angle):
        return self.rotated(_AXES["x"], angle)

    def rotated_y(self, angle):
        return self.rotated(_AXES["y"], angle)

    def rotated_z(self, angle):
        return self.rotated(_AXES["z"], angle)


class BomItem:
    """One line of a bill of materials: a distinct part and how many instances of it there are."""

    def __init__(self, name, part):
        self.name = name
        self.part = part
        self.count = 1

    def shape(self):
        """The part's shape, unplaced (lets a BOM item be rendered like a shape)."""
        return self.part.data

    def __str__(self):
        return "{}x {}".format(self.count, self.name)


class _AssemblyMixin:
    """What a placed assembly adds to an instance: its contents, flattened, counted and united."""

    __slots__ = ()

    def __iter__(self):
        """The instances listed directly in this assembly (subassemblies are not entered)."""
        return iter(self.part.instances)

    def all_instances(self):
        """Every part instance of this assembly, subassemblies entered recursively, in listing order.  The
        transforms of the enclosing subassemblies are composed into each instance, so it stands where it stands
        in this assembly's frame (the assembly's own transform is not applied, as for its direct instances); the
        instances of a hidden subassembly are hidden."""
        for instance in self:
            if isinstance(instance, _AssemblyMixin):
                for inner in instance.all_instances():
                    inner = inner._transformed(instance.transform)
                    yield inner if instance.visible else inner.hidden()
            else:
                yield instance

    def bom(self, recursive=True, visible_only=False):
        """BomItems in order of first appearance.  recursive=False counts the direct instances (a subassembly is
        one item).  Instances of the same Part object share an item; distinct parts that share a name get items
        named name, name-2, name-3, ... in that order."""
        by_name = collections.OrderedDict()
        for instance in (self.all_instances() if recursive else self):
            if visible_only and not instance.visible:
                continue
            items = by_name.setdefault(instance.part.name, [])
            for item in items:
                if item.part is instance.part:
                    item.count += 1
                    break
            else:
                suffix = "-{}".format(len(items) + 1) if items else ""
                items.append(BomItem(instance.part.name + suffix, instance.part))
        for items in by_name.values():
            yield from items

    def shape(self):
        """The union of the visible instances (hidden ones are left out), in this assembly's placement."""
        from . import shapes
        united = shapes.union(instance.shape() for instance in self.all_instances() if instance.visible)
        if self.transform == util.Transformation.zero():
            return united
        return united.transformed(self.transform)


class AssemblyTransform2D(_AssemblyMixin, PartTransform2D):
    __slots__ = ()


class AssemblyTransform3D(_AssemblyMixin, PartTransform3D):
    __slots__ = ()


def assembly(name, instances, attributes=None):
    """A new assembly of `instances` (parts from `Shape*.make_part` or other assemblies), placed at the origin
    and visible.  Raises ValueError when `instances` is empty or mixes 2D and 3D."""
    instances = list(instances)
    if not instances:
        raise ValueError("An assembly needs at least one instance")
    dimensions = {instance.dimension() for instance in instances}
    if len(dimensions) > 1:
        raise ValueError("An assembly cannot mix 2D and 3D instances")
    cls = AssemblyTransform2D if dimensions == {2} else AssemblyTransform3D
    return cls(Assembly(name, instances, list(attributes or [])), util.Transformation.zero(), True)


def make_part(shape, name, attributes=None):
    """`shape` as a part instance at the origin (Shape2D.make_part / Shape3D.make_part)."""
    cls = PartTransform2D if shape.dimension() == 2 else PartTransform3D
    return cls(Part(name, shape, list(attributes or [])), util.Transformation.zero(), True)
